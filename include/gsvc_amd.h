/*
 * gsvc_amd.h -- C ABI of the MI355X-native 2D Gaussian-splat rasterizer.
 *
 * This is the drop-in boundary for the hot path of ac-freeman/GSVC: the ops
 * that the reference's torch extension ``gsplat.csrc`` exports
 * (gsplat/gsplat/cuda/csrc/ext.cpp:6-23, prototypes bindings.h:16-301) for the
 * 2D path, plus the binning glue the reference ran in PyTorch
 * (gsplat/gsplat/utils.py:99-167).  Every entry point takes plain device
 * pointers and sizes; no torch types cross it.  The Python mirror of the
 * reference operator API (gsvc_amd/, re-exported as the ``gsplat`` package)
 * binds these with ctypes; INTEGRATION.md shows the binding a maintainer of
 * the reference would add.
 *
 * Conventions
 *   - All pointers are device (HBM) pointers unless stated otherwise.
 *   - ``stream`` is a hipStream_t (NULL = legacy default stream); every entry
 *     point is asynchronous on it and never synchronises the device, so calls
 *     can be captured in a hipGraph -- except the entries whose workspace
 *     alternates host-indexed parity slots (call_index / frame_index: the
 *     slab renders, gsvc_rasterize_sum_forward_slabs*, the fused training
 *     step): a replay would re-add into the slots capture froze, so they
 *     refuse a capturing stream with GSVC_ERR_CAPTURE before any launch (the
 *     reference's own forward cannot be captured either: its .item(),
 *     utils.py:117).  The counted binning + rasterize_sum entries are the
 *     capturable route.
 *   - Return value: 0 on success, otherwise a gsvc_status code; the message of
 *     the last failure on the calling thread is gsvc_last_error().  Bad
 *     arguments are rejected before any launch (the reference raised
 *     c10::Error through TORCH_CHECK / AT_ERROR, bindings.h:9-14).
 *   - Outputs are fully written by the call (no caller-side zeroing needed)
 *     unless a comment says otherwise.
 *   - Images are row-major HWC float32, pixel (j, i) evaluated at (j, i).
 *   - Only 16x16 tiles are supported (the reference kernels hard-code
 *     BLOCK_X = BLOCK_Y = 16, config.h:1-4).
 */
#ifndef GSVC_AMD_H
#define GSVC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum gsvc_status {
    GSVC_OK = 0,
    GSVC_ERR_ARG = 1,       /* invalid argument (shape, size, tile size) */
    GSVC_ERR_WORKSPACE = 2, /* workspace too small */
    GSVC_ERR_HIP = 3,       /* HIP runtime / launch error */
    GSVC_ERR_CAPTURE = 4    /* the stream is capturing a graph and the entry keeps host-indexed state */
};

/* ABI version 2: gsvc_debug_set / gsvc_debug_set_ptr moved to the diagnostic
 * library (gsvc_amd_diag.h); GSVC_ERR_CAPTURE added.
 * ABI version 3: gsvc_encode_stream_bytes / gsvc_encode_stream added.
 * ABI version 4: gsvc_quant_train_workspace_bytes / gsvc_quant_train_step /
 * gsvc_quant_adan_step added.  gsvc_rgb_to_i420 and gsvc_quant_train_run joined
 * version 4 later, and after them gsvc_yuv_format_table, gsvc_yuv420_to_rgb and
 * gsvc_rgb_to_yuv420, then gsvc_yuv_to_rgb and gsvc_rgb_to_yuv: added entries,
 * nothing existing changed. */
#define GSVC_ABI_VERSION 4

/* Library identity and error reporting. */
int gsvc_abi_version(void);
const char *gsvc_last_error(void);

/* ---------------------------------------------------------------------------
 * Fused Adan step (optimizer.py:296-362 _multi_tensor_adan, one kernel for
 * all tensors).  Host arrays of ntensors device pointers / element counts;
 * every tensor contiguous fp32.  Scalars as in the reference (bias
 * corrections computed by the caller, optimizer.py:171-173,211).  grads are
 * read, not scaled in place. */
int gsvc_adan_step(int ntensors, const long long *numels, float *const *params,
                   const float *const *grads, float *const *exp_avgs,
                   float *const *exp_avg_sqs, float *const *exp_avg_diffs,
                   float *const *neg_pre_grads, double beta1, double beta2, double beta3,
                   double bias_correction1, double bias_correction2,
                   double bias_correction3_sqrt, double lr, double weight_decay, double eps,
                   int no_prox, double clip_global_grad_norm, void *stream);

/* ---------------------------------------------------------------------------
 * Pruning of a frame model (GaussianSplats_Represent.py:101-125 removal_control
 * and :149-166 adaptive_control: norm of rgb_W, torch.sort, boolean-mask
 * rebuild of _xyz / _cholesky / _features_dc / rgb_W).  Removes the
 * remove_count splats of smallest ||rgb_W|| (rgb_w: fp32 [num_points, 1];
 * equal norms leave in index order, as the GPU's stable torch.sort) and writes
 * the kept rows, in order, of each of the ntensors fp32 [num_points, cols[t]]
 * tensors src[t] to dst[t] ([num_points - remove_count, cols[t]]; src and dst
 * must not overlap).  Host arrays of device pointers; no host sync.
 * remove_count >= num_points keeps nothing and launches nothing. */
size_t gsvc_prune_workspace_bytes(int num_points);
int gsvc_prune_lowest(int num_points, int remove_count, const float *rgb_w, int ntensors,
                      const int *cols, const float *const *src, float *const *dst,
                      void *workspace, size_t workspace_bytes, void *stream);

/* Launch timing of the sum-forward composite kernel (every rasterizer entry
 * point above): after gsvc_timing_enable(max, every, how), every every-th
 * launch is timed by HIP events on its stream (up to max launches) -- how = 0:
 * events recorded before and after the launch (includes the marker packets and
 * the dispatch, ~3 us); how = 1: events carried by the dispatch itself
 * (hipExtLaunchKernel: the kernel's own start / end, as a kernel trace).
 * gsvc_timing_collect waits for them and writes the durations in ms.
 * gsvc_timing_enable(0, 0, 0) stops and frees.  Not part of the reference. */
int gsvc_timing_enable(int max_launches, int every, int how);
int gsvc_timing_collect(float *ms, int max_out, int *count);
/* The same for one kernel channel: 0 the composite (as above), 1 the fused
 * training step's tile kernel, 2 the frame projection (render and training),
 * 3 the training step's per-splat kernel (projection VJP + Adan), 4 the sum
 * rasterizer's backward, 5 / 6 the alpha rasterizer's forward / backward. */
int gsvc_timing_enable_channel(int channel, int max_launches, int every, int how);
int gsvc_timing_collect_channel(int channel, float *ms, int max_out, int *count);

/* The unit-opacity alpha cut as a sigma threshold (alpha_cut.hip): the
 * kernels' constant, and a device scan over all 2^31 non-negative float
 * patterns of the reference predicate (forward.cu:598-606 at opacity 1) into
 * out[4] (device memory) = {largest kept, smallest dropped, kept with
 * exp(-sigma) > 1, kept NaN patterns}.  Test hooks; not part of the reference. */
unsigned gsvc_alpha_cut_bits(void);
int gsvc_alpha_cut_scan(unsigned *out, void *stream);

/* hipStreamSynchronize(stream): the fused training step writes its losses
 * into caller memory that may be pinned host memory; the caller waits with
 * this before reading them (the reference's PSNR .item(),
 * GaussianSplats_Represent.py:196-198).  Not part of the reference. */
int gsvc_stream_sync(void *stream);
/* Coherent pinned host memory (hipHostMallocCoherent), zeroed: a kernel's
 * system-scope stores to it are seen by the host while the kernel runs.
 * Not part of the reference. */
void *gsvc_host_alloc(size_t bytes);
int gsvc_host_free(void *p);
/* Spin until the unsigned at ``word`` (coherent host memory) equals ``seq``;
 * after spin_us microseconds fall back to gsvc_stream_sync(stream), which
 * reports a failed kernel, and then require it.  The fused training step's
 * early loss read-back (GSVC_TRAIN_LOSS_SEQ).  Not part of the reference. */
int gsvc_wait_host_seq(const unsigned *word, unsigned seq, void *stream, int spin_us);

/* ---------------------------------------------------------------------------
 * 2D projection.
 * Replaces _C.project_gaussians_2d_forward
 *   (bindings.cu:781-839 -> foward2d.cu:12-69; Python project_gaussians_2d.py:63-103).
 * means2d [N,2], L_elements [N,3] (l11, l21, l22) in; xys [N,2], depths [N]
 * (all 0), radii [N] int32, conics [N,3], num_tiles_hit [N] int32 out.
 * clip_thresh is accepted and unused, as in the reference.
 */
int gsvc_project_gaussians_2d_forward(
    int num_points, const float *means2d, const float *L_elements,
    unsigned img_height, unsigned img_width,
    int tile_bounds_x, int tile_bounds_y, int tile_bounds_z, float clip_thresh,
    float *xys, float *depths, int *radii, float *conics, int *num_tiles_hit,
    void *stream);

/* Replaces _C.project_gaussians_2d_backward
 *   (bindings.cu:902-949 -> backward2d.cu:8-51; Python project_gaussians_2d.py:105-141).
 * v_depth is accepted and unused, as in the reference.  The L gradient keeps
 * the reference's doubled off-diagonal term (backward2d.cu:39-41). */
int gsvc_project_gaussians_2d_backward(
    int num_points, const float *means2d, const float *L_elements,
    unsigned img_height, unsigned img_width,
    const int *radii, const float *conics,
    const float *v_xy, const float *v_depth, const float *v_conic,
    float *v_cov2d, float *v_mean2d, float *v_L_elements,
    void *stream);

/* The same backward with row strides for v_xy and v_conic (>= 2 and >= 3
 * floats): the rasterizer backward's gradient records ([N,16], v_xy at 0,
 * v_conic at 2) are read in place, without a contiguous copy.  means2d and
 * v_depth, unused by the reference kernel, are not taken.  Not part of the
 * reference (the autograd Function of csrc/torch_ops.cpp calls it). */
int gsvc_project_gaussians_2d_backward_strided(
    int num_points, const float *L_elements, unsigned img_height, unsigned img_width,
    const int *radii, const float *conics, const float *v_xy, int v_xy_stride,
    const float *v_conic, int v_conic_stride, float *v_cov2d, float *v_mean2d,
    float *v_L_elements, void *stream);

/* Replaces _C.compute_cov2d_bounds (bindings.cu:41-60 -> :21-39).
 * covs2d [N,3] upper-triangular in; conics [N,3], radii [N] float out. */
int gsvc_compute_cov2d_bounds(int num_pts, const float *covs2d, float *conics,
                              float *radii, void *stream);

/* ---------------------------------------------------------------------------
 * Binning.  Replaces the torch glue of utils.py:99-167 and the two binning
 * ops _C.map_gaussian_to_intersects / _C.get_tile_bin_edges.
 */

/* torch.cumsum(num_tiles_hit, dtype=int32) of utils.py:116, plus a 4-int
 * device record ``meta`` = {M = cum[N-1], OR of depth bits, AND of depth bits,
 * splats with num_tiles_hit > 0} over the splats that emit intersections.
 * ``depths`` may be NULL (then meta[1] = meta[2] = 0).  Reading meta[0] on the
 * host is the one device->host sync of the forward (utils.py:117 ``.item()``). */
size_t gsvc_cumsum_workspace_bytes(int num_points);
int gsvc_compute_cumulative_intersects(
    int num_points, const int *num_tiles_hit, const float *depths,
    int *cum_tiles_hit, int *meta, void *workspace, size_t workspace_bytes,
    void *stream);

/* Replaces _C.map_gaussian_to_intersects (bindings.cu:274-313 -> forward.cu:100-136).
 * isect_ids [M] int64 = tile_id << 32 | sign-extended depth bits, gaussian_ids [M] int32. */
int gsvc_map_gaussian_to_intersects(
    int num_points, int num_intersects, const float *xys, const float *depths,
    const int *radii, const int *cum_tiles_hit,
    int tile_bounds_x, int tile_bounds_y, int tile_bounds_z,
    int64_t *isect_ids, int *gaussian_ids, void *stream);

/* Replaces torch.sort(isect_ids) + torch.gather(gaussian_ids) (utils.py:164-165):
 * stable LSD radix sort of signed int64 keys on bits [begin_bit, end_bit)
 * (pass 0, 64 for a full sort).  Keys equal on those bits keep input order. */
size_t gsvc_sort_pairs_workspace_bytes(int n);
int gsvc_sort_isect_pairs(
    int n, const int64_t *keys_in, const int *vals_in,
    int64_t *keys_out, int *vals_out, int begin_bit, int end_bit,
    void *workspace, size_t workspace_bytes, void *stream);

/* Replaces _C.get_tile_bin_edges (bindings.cu:315-330 -> forward.cu:141-163).
 * tile_bins [rows,2] int32 is zeroed then filled; rows must exceed every tile
 * id present (the reference allocated M rows, which overflowed when M < tiles). */
int gsvc_get_tile_bin_edges(int num_intersects, const int64_t *isect_ids_sorted,
                            int *tile_bins, int rows, void *stream);

/* Fused hot-path binning used by rasterize_gaussians_sum (utils.py:121-167 in
 * one call): emit (tile, splat) pairs in splat order, stable radix sort on the
 * ceil(log2(tiles)) tile bits only, and bin edges.  Valid when every emitting
 * splat has the same depth bits (meta[1] == meta[2]; always true for the 2D
 * projection, which writes depth 0), which makes the reference's 64-bit order
 * equal to the tile order.  gaussian_ids_sorted [M]; tile_bins [rows,2] with
 * rows >= tiles; isect_ids_sorted [M] optional (NULL to skip). */
size_t gsvc_bin_tiles_workspace_bytes(int num_points, int num_intersects, int num_tiles);
int gsvc_bin_and_sort_tiles(
    int num_points, int num_intersects, const float *xys, const float *depths,
    const int *radii, const int *cum_tiles_hit,
    int tile_bounds_x, int tile_bounds_y,
    int *gaussian_ids_sorted, int *tile_bins, int tile_bins_rows,
    int64_t *isect_ids_sorted, void *workspace, size_t workspace_bytes,
    void *stream);

/* Sync-free tile binning used by the rasterizer ops (the hot path of
 * utils.py:99-167 + bindings.cu:274-330 without reading num_intersects on the
 * host): builds gaussian_ids_sorted in the stable (tile, splat id) order of
 * the reference's sorted pairs and tile_bins[tbx*tby] ([start,end), (0,0)
 * when empty), every size staying on the device.  meta[0] <- M,
 * meta[1] <- 1 if the entries kept exceed capacity (outputs then
 * incomplete: a tile whose segment ends past capacity is neither sorted nor,
 * with tile_cap, rebuilt; no element at or past capacity is written).
 * ids_scratch and gaussian_ids_sorted hold >= capacity ints.
 * tile_cap > 0 keeps only each tile's first tile_cap entries in id order (the
 * sum rasterizer reads no more than 256 per tile, forward.cu:569-571,613; a
 * tile with more is rebuilt from the splats' bboxes in id order), so
 * capacity = tiles * min(num_points, tile_cap) can never overflow; with
 * tile_cap 0 every entry is kept and capacity = num_points * tiles is the
 * safe bound.  M is the uncapped total either way.  Deterministic. */
size_t gsvc_bin_tiles_counted_workspace_bytes(int num_tiles);
int gsvc_bin_tiles_counted(int num_points, const float *xys, const int *radii,
                           int tile_bounds_x, int tile_bounds_y, long long capacity,
                           int tile_cap, int *ids_scratch, int *gaussian_ids_sorted,
                           int *tile_bins, int *meta, void *workspace,
                           size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Sum rasterizer (the GSVC renderer, rasterize_sum.py).
 * Replaces _C.rasterize_sum_forward (bindings.cu:400-469 -> forward.cu:512-627):
 * out[p] = sum over the first <= 256 sorted entries k of p's tile of
 * colors[g_k] * min(1, opac[g_k] * exp(-sigma)), skipping sigma < 0 and
 * alpha < 1/255; final_idx[p] = last contributing k (0 if none); final_Ts = 1.
 * final_Ts may be NULL (it is identically 1; the Python layer returns an
 * expanded constant).  background is accepted and unused, as in the reference. */
int gsvc_rasterize_sum_forward(
    int tile_bounds_x, int tile_bounds_y, int tile_bounds_z,
    int block_x, int block_y, int block_z,
    unsigned img_width, unsigned img_height, unsigned img_depth,
    const int *gaussian_ids_sorted, const int *tile_bins,
    const float *xys, const float *conics, const float *colors,
    const float *opacities, const float *background,
    float *out_img, float *final_Ts, int *final_idx, void *stream);

/* The same op with the knobs of the sync-free hot path (results identical to
 * gsvc_rasterize_sum_forward for the same inputs):
 *   num_intersects_dev  device int M (NULL: M > 0 assumed); when M < 1 every
 *                       pixel gets background, the reference's M < 1 branch
 *                       (rasterize_sum.py:121-127), final_idx 0;
 *   density_hint        an estimate of M (any value is correct; > 5 entries
 *                       per tile selects the banded two-waves-per-tile
 *                       kernel, otherwise one wave per tile);
 *   out_layout          0: out_img [H,W,3] as the reference;
 *                       1: out_img [3,H,W] = torch.clamp(img, 0, 1) permuted,
 *                       the caller epilogue of GaussianSplats_Represent.py:88-89;
 *                       2: out_img as channel planes [3,H,W], unclamped: the
 *                       [H,W,3] image with strides (W, 1, H*W) (GSVC_SLABS_PLANES);
 *   final_idx, final_Ts may be NULL (not written). */
int gsvc_rasterize_sum_forward_ex(
    int tile_bounds_x, int tile_bounds_y, int tile_bounds_z,
    int block_x, int block_y, int block_z,
    unsigned img_width, unsigned img_height, unsigned img_depth,
    const int *gaussian_ids_sorted, const int *tile_bins,
    const float *xys, const float *conics, const float *colors,
    const float *opacities, const float *background,
    const int *num_intersects_dev, int density_hint, int out_layout,
    float *out_img, float *final_Ts, int *final_idx, void *stream);

/* The op path's binning and composite in two kernels, no host sync and no
 * sort kernels: rasterize_sum.py:110-136's cumsum + map + sort + bin edges
 * (utils.py:99-167; forward.cu:100-163) and rasterize_forward_sum
 * (forward.cu:512-627).  Every visible splat appends its id to a 256-slot id
 * slab of each tile of its bbox (device atomics); the composite sorts a
 * tile's ids in LDS -- the first <= 256 in (tile, splat id) order, as the
 * reference's stable sort of (tile << 32 | depth 0) keys gives -- blends them
 * and writes them back sorted: gaussian_ids [T * 256] (tile t's at t * 256)
 * and tile_bins [T, 2] = [t * 256, t * 256 + n) are then the inputs of the
 * backward.  final_idx (optional; NULL: not written -- the backward below
 * needs none when the forward was this one) indexes gaussian_ids.  meta[0] <- M (device), meta[1] <-
 * 0; M < 1 renders the background (rasterize_sum.py:121-127).
 * grad_records_zero (optional, [N, 16]) is zeroed for
 * gsvc_rasterize_sum_backward_zeroed.  workspace: the first
 * gsvc_rasterize_sum_slabs_workspace_bytes(T) bytes must be zero before the
 * first call with it; each call (call_index = a counter, alternate parities)
 * leaves them ready for the next.  Requires every splat's depth to be 0
 * (project_gaussians_2d's output).  Not part of the reference. */
size_t gsvc_rasterize_sum_slabs_workspace_bytes(int num_tiles);
int gsvc_rasterize_sum_forward_slabs(
    int num_points, const float *xys, const int *radii, const float *conics,
    const float *colors, const float *opacities, const float *background,
    unsigned img_height, unsigned img_width, int call_index, int density_hint,
    void *workspace, size_t workspace_bytes, int *gaussian_ids, int *tile_bins,
    int *meta, float *grad_records_zero, float *out_img, int *final_idx, void *stream);
/* The same with a splat order for the id insertion (speed only; the same
 * results): order_flags GSVC_TRAIN_ORDER inserts the splats in the order an
 * earlier GSVC_TRAIN_ORDER_REFRESH call with this order_workspace and
 * num_points sorted (by the tile strip of their centres), so a workgroup's
 * slot atomics aggregate per tile; GSVC_TRAIN_ORDER_REFRESH sorts a new one
 * from this call's xys.  order_workspace: gsvc_rasterize_sum_order_workspace_bytes
 * (num_points) bytes, no initial contents.  order_flags GSVC_SLABS_WIDE (with
 * or without an order): gaussian_ids holds GSVC_SLABS_WIDE_IDS ids per tile
 * ([T * 1024], tile t's at t * 1024, tile_bins [t * 1024, t * 1024 + n)): a
 * tile of up to 1024 entries sorts its first 256 from its slab instead of
 * rebuilding them from every splat's bbox (dense content).  order_flags
 * GSVC_SLABS_PLANES: out_img is written as channel planes [3, H, W] (unclamped;
 * the same values as the [H, W, 3] image, element (i, j, c) at c*H*W + i*W + j)
 * -- the layout GSVC's own epilogue (clamp, view, permute(0, 3, 1, 2),
 * contiguous; GaussianSplats_Represent.py:88-89) reads without a copy.  Not
 * part of the reference. */
#define GSVC_SLABS_WIDE 0x80000
#define GSVC_SLABS_PLANES 0x100000
#define GSVC_SLABS_WIDE_IDS 1024
size_t gsvc_rasterize_sum_order_workspace_bytes(int num_points);
int gsvc_rasterize_sum_forward_slabs_ordered(
    int num_points, const float *xys, const int *radii, const float *conics,
    const float *colors, const float *opacities, const float *background,
    unsigned img_height, unsigned img_width, int call_index, int density_hint,
    void *workspace, size_t workspace_bytes, int *gaussian_ids, int *tile_bins,
    int *meta, float *grad_records_zero, float *out_img, int *final_idx, void *stream,
    void *order_workspace, size_t order_workspace_bytes, int order_flags);
/* gsvc_rasterize_sum_backward (backward.cu:696-862) into grad_records that
 * the caller has zeroed (gsvc_rasterize_sum_forward_slabs did): no memset.
 * final_idx [H, W] (indices into gaussian_ids_sorted): when given, pixel p
 * skips every entry k > final_idx[p], as the reference does
 * (backward.cu:783-786), whatever forward produced it.  NULL: no per-pixel
 * bound is read -- valid ONLY for the final_idx that this library's own sum
 * forward kernels imply (an entry past a pixel's last contributor fails the
 * alpha test there in the same op sequence); a forward with another alpha
 * test (e.g. a fast-math build) must pass its final_idx. */
int gsvc_rasterize_sum_backward_zeroed(
    unsigned img_height, unsigned img_width, int num_points,
    const int *gaussian_ids_sorted, const int *tile_bins, const float *xys,
    const float *conics, const float *colors, const float *opacities,
    const int *final_idx, const float *v_output, float *grad_records, void *stream);
/* The same with v_output at any strides (in floats; element (row i, column j,
 * channel c) at v_output[i * v_stride_h + j * v_stride_w + c * v_stride_c]):
 * the autograd engine's gradient as it arrives -- after GSVC's
 * permute(0, 3, 1, 2) it is channel planes -- read without a copy
 * (rasterize_sum.py:189-254 calls .contiguous()).  Not part of the reference. */
int gsvc_rasterize_sum_backward_zeroed_strided(
    unsigned img_height, unsigned img_width, int num_points,
    const int *gaussian_ids_sorted, const int *tile_bins, const float *xys,
    const float *conics, const float *colors, const float *opacities,
    const int *final_idx, const float *v_output, long long v_stride_h,
    long long v_stride_w, long long v_stride_c, float *grad_records, void *stream);
/* The same with flags: GSVC_BWD_NO_OPACITY -- the caller's opacities take no
 * gradient (GSVC's constant ones, GaussianSplats_Represent.py:84): v_opacity
 * (record word 8) is neither computed nor written, and each (splat, tile)
 * request covers the record's first 32 bytes.  Not part of the reference. */
#define GSVC_BWD_NO_OPACITY 0x1
int gsvc_rasterize_sum_backward_zeroed_strided_ex(
    unsigned img_height, unsigned img_width, int num_points,
    const int *gaussian_ids_sorted, const int *tile_bins, const float *xys,
    const float *conics, const float *colors, const float *opacities,
    const int *final_idx, const float *v_output, long long v_stride_h,
    long long v_stride_w, long long v_stride_c, float *grad_records, void *stream, int flags);

/* ---------------------------------------------------------------------------
 * Whole-frame render of GSVC's per-frame model (GaussianSplats_Represent.py:
 * 57-90) in one call (two kernels), no host synchronisation: out[3,H,W] =
 * clamp(rasterize_gaussians_sum(project_gaussians_2d(means2d, L)), 0, 1)
 * permuted to planes, with
 *   means2d = xyz_tanh ? tanh(xyz) : xyz            xyz [N,2]
 *   L       = cholesky + cholesky_bound (if given)   cholesky [N,3], bound [3]
 *   colors  = features * rgb_w (if given)            features [N,3], rgb_w [N]
 *   opacity = opacity (if given) else 1              [N]
 * Results are bit-identical to the op path.  meta (device int[2]) <- {M, 0}.
 * The workspace (gsvc_render_frame_workspace_bytes) must have its first
 * gsvc_render_frame_zeroed_bytes zero before the first call; every call leaves
 * them zero.  frame_index: any integer that alternates parity between
 * consecutive calls on one workspace (a frame counter).  density_hint as in
 * gsvc_rasterize_sum_forward_ex. */
size_t gsvc_render_frame_workspace_bytes(int num_points, unsigned img_height,
                                         unsigned img_width);
size_t gsvc_render_frame_zeroed_bytes(unsigned img_height, unsigned img_width);
int gsvc_render_frame_sum(int num_points, const float *xyz, int xyz_tanh,
                          const float *cholesky, const float *cholesky_bound,
                          const float *features, const float *rgb_w,
                          const float *opacity, const float *background,
                          unsigned img_height, unsigned img_width, int frame_index,
                          int density_hint, int *meta, void *workspace,
                          size_t workspace_bytes, float *out, void *stream);
/* The same with ``flags``: GSVC_TRAIN_ORDER / GSVC_TRAIN_ORDER_REFRESH (below)
 * project in / refresh the workspace's splat order, as the training step does
 * (speed only: the same image).  Not part of the reference. */
int gsvc_render_frame_sum_ex(int num_points, const float *xyz, int xyz_tanh,
                             const float *cholesky, const float *cholesky_bound,
                             const float *features, const float *rgb_w,
                             const float *opacity, const float *background,
                             unsigned img_height, unsigned img_width, int frame_index,
                             int density_hint, int *meta, void *workspace,
                             size_t workspace_bytes, float *out, void *stream, int flags);

/* ---------------------------------------------------------------------------
 * Fused training step of GSVC's per-frame model: one
 * GaussianVideo_frame.train_iter (GaussianSplats_Represent.py:191-207) with
 * the L2 (loss_kind 0, F.mse_loss) or L1 (loss_kind 1, F.l1_loss) loss and
 * Adan (optimizer.py:124-235, 296-362), in three kernels, no host sync:
 *   forward  means2d = tanh(xyz), L = cholesky + cholesky_bound (if given),
 *            colors = features * rgb_w (if given), opacity 1; the sum
 *            rasterizer; clamp(0, 1) -- the same image bits as
 *            gsvc_render_frame_sum (render_out [3,H,W], optional);
 *   loss     against gt [3,H,W]; loss[0] <- mean squared error (the PSNR's
 *            MSE), loss[1] <- mean absolute error; ``loss`` may be device
 *            memory or pinned host memory (written by the last kernel; read
 *            it after gsvc_stream_sync);
 *   backward through clamp, rasterizer, projection (doubled L cross term,
 *            backward2d.cu:39-41) and the activations;
 *   Adan     every element of xyz [N,2], cholesky [N,3], features [N,3] and,
 *            when rgb_w_trainable, rgb_w [N] is updated in place.
 * adan_state: host array of 16 device pointers, per parameter (xyz,
 * cholesky, features, rgb_w) its {exp_avg, exp_avg_sq, exp_avg_diff,
 * neg_pre_grad} (rgb_w's may be NULL when not trainable).  adan_hparams: host
 * double[10] = {beta1, beta2, beta3, bias_correction1, bias_correction2,
 * sqrt(bias_correction3), lr, weight_decay, eps, clip_global_grad_norm}.
 * adan_flags: bit 0 no_prox; bit 1 + q: parameter q takes its first step
 * (neg_pre_grad starts from -grad, optimizer.py:187-189); GSVC_TRAIN_LOSS_SEQ:
 * ``loss`` is coherent host memory (gsvc_host_alloc) of at least 3 words and,
 * once loss[0..1] are stored, word 2 receives (frame_index + 1) | 0x80000000
 * with a system-scope release -- the host may read the losses then
 * (gsvc_wait_host_seq) while the rest of the step still runs; every later
 * operation on ``stream`` sees the updated parameters.
 * grads_out (test hook): when non-NULL nothing is updated and the parameter
 * gradients go to grads_out [N,9] = {d_xyz 2, d_cholesky 3, d_features 3,
 * d_rgb_w 1}.  Workspace: gsvc_train_step_workspace_bytes; its first
 * gsvc_render_frame_zeroed_bytes(H, W) bytes zero before the first call (every
 * call leaves them zero); frame_index alternates parity between calls.
 *
 * Weighted Y/U/V loss (loss_kind 2, gsvc_train_step_sum_args only; not part of
 * the reference): with x = clamp(render, 0, 1), d = x - gt, the 3x3
 * RGB -> (Y, U, V) matrix M and weights w of ``loss_yuv``, e_k = sum_c
 * M[k][c] d_c per pixel, Y per pixel and U, V averaged over the chroma block
 * of ``loss_chroma`` (2x2 at 4:2:0, 2x1 at 4:2:2, 1x1 at 4:4:4, aligned to
 * even coordinates), the loss is
 *   L = sum_k w_k mse_k / sum_k w_k,  mse_k = mean over blocks of (block mean e_k)^2,
 * and its gradient passes the clamp where 0 <= render <= 1.  loss[0] stays
 * the RGB mean squared error (the PSNR's), loss[1] <- L.  Weights are finite,
 * non-negative, with a positive sum; 4:2:0 needs even img_height and
 * img_width, 4:2:2 an even img_width (GSVC_ERR_ARG otherwise). */
#define GSVC_TRAIN_LOSS_SEQ 0x100
/* Splat order (speed only; the same results): GSVC_TRAIN_ORDER projects the
 * splats in the order an earlier GSVC_TRAIN_ORDER_REFRESH call of the same
 * workspace, num_points and image size sorted (by the tile strip of their
 * centres), so a workgroup's slot atomics aggregate per tile;
 * GSVC_TRAIN_ORDER_REFRESH sorts a new one from this call's positions. */
#define GSVC_TRAIN_ORDER 0x200
#define GSVC_TRAIN_ORDER_REFRESH 0x400
/* Projection placement (speed only): by default a call projects its frame
 * first.  GSVC_TRAIN_PROJECT_ONLY: project frame_index and return (the order
 * flags apply to it).  GSVC_TRAIN_PROJECTED: this frame's projection was
 * already enqueued on the stream by the previous call's
 * GSVC_TRAIN_PROJECT_NEXT, which (requiring PROJECTED) enqueues the projection
 * of frame_index + 1 -- from the parameters this step updates -- after the
 * step, so it follows the step on the device without waiting for the host; the
 * order flags then apply to that projection.  The caller guarantees that
 * nothing changes the parameters between the two calls (or discards the
 * pending projection by re-zeroing the workspace). */
#define GSVC_TRAIN_PROJECT_ONLY 0x800
#define GSVC_TRAIN_PROJECTED 0x1000
#define GSVC_TRAIN_PROJECT_NEXT 0x2000
/* GSVC_TRAIN_DETERMINISTIC (gsvc_train_step_sum_args only): bitwise
 * reproducible gradients.  The tile kernel writes each (splat, tile) gradient
 * sum -- itself formed in a fixed order -- to its own slot instead of adding
 * it with float atomics (backward.cu:843-859 uses atomics, so the reference
 * is not reproducible run to run), and the splat kernel adds a splat's slots
 * in tile-bbox row-major order.  Needs det_workspace of
 * gsvc_train_step_det_workspace_bytes(num_points, det_capacity) bytes;
 * det_capacity (>= the frame's M, the (splat, tile) pairs) slots of 32 B.
 * Pairs past the capacity fall back to the atomics (correct, not
 * reproducible).  With GSVC_TRAIN_LOSS_SEQ, ``loss`` then holds 4 words and
 * word 3 receives the frame's M (before the sequence word), so the caller can
 * grow det_capacity. */
#define GSVC_TRAIN_DETERMINISTIC 0x4000
/* GSVC_TRAIN_CARRY (speed only; the same results): carried bins.  The tile
 * bins are kept from step to step instead of re-projected: with
 * GSVC_TRAIN_PROJECT_ONLY (or a call without GSVC_TRAIN_PROJECTED) the
 * projection builds them -- per tile the ids of the splats whose tile box
 * holds it -- and a step with GSVC_TRAIN_PROJECTED | GSVC_TRAIN_CARRY reads
 * them, keeping of each tile's candidates those whose current box holds the
 * tile, while its splat kernel, right after a splat's Adan update, projects the
 * splat for frame_index + 1 and appends its id to the tiles its box newly
 * reaches (the bins only grow: stale candidates are skipped).  Each step thus
 * leaves the next frame projected and binned, with no projection kernel.  The
 * caller rebuilds them now and then (a PROJECT_ONLY call) and whenever the
 * parameters changed outside the steps, as for GSVC_TRAIN_PROJECT_NEXT, which
 * it excludes. */
#define GSVC_TRAIN_CARRY 0x8000
/* Tile kernel ahead (speed only; the same results; with CARRY | PROJECTED and
 * the Adan update, not with render_out; with DETERMINISTIC the next call must
 * pass the same det_workspace and det_capacity).
 * GSVC_TRAIN_TILES_NEXT: after the step, enqueue frame_index + 1's tile kernel
 * (forward, loss and backward into the workspace's gradient records and tile
 * errors) against this call's ``gt`` -- it reads the bins and records this
 * step's splat kernel carried, and none of the next call's hyper-parameters --
 * so the device starts the next iteration while the host is still returning
 * this one's loss.  GSVC_TRAIN_TILED: this frame's tile kernel is the one the
 * previous call enqueued; the call launches the splat kernel (the loss, the
 * Adan update with this call's hyper-parameters, the carry).  The caller
 * guarantees that neither the parameters nor gt (nor background) changed
 * between the two calls; otherwise it discards the pending kernel's work by
 * rebuilding (re-zeroing the workspace and a PROJECT_ONLY call, which also
 * zeroes the gradient records). */
#define GSVC_TRAIN_TILES_NEXT 0x10000
#define GSVC_TRAIN_TILED 0x20000
/* GSVC_TRAIN_REBUILD_NEXT (with TILES_NEXT): rebuild frame_index + 1's carried
 * bins from scratch (the PROJECT_ONLY | CARRY projection of the updated
 * parameters; the order flags apply to it) before enqueueing its tile kernel --
 * the periodic rebuild without a host round trip. */
#define GSVC_TRAIN_REBUILD_NEXT 0x40000
size_t gsvc_train_step_det_workspace_bytes(int num_points, long long det_capacity);
size_t gsvc_train_step_workspace_bytes(int num_points, unsigned img_height,
                                       unsigned img_width);
int gsvc_train_step_sum(int num_points, float *xyz, float *cholesky,
                        const float *cholesky_bound, float *features, float *rgb_w,
                        int rgb_w_trainable, const float *background, const float *gt,
                        unsigned img_height, unsigned img_width, int loss_kind,
                        int frame_index, float *const *adan_state,
                        const double *adan_hparams, int adan_flags, float *loss,
                        float *render_out, float *grads_out, void *workspace,
                        size_t workspace_bytes, void *stream);
/* gsvc_train_step_sum with its arguments in one struct (the same names and
 * meaning): a binding that keeps the struct across calls and updates only
 * what changes pays one argument conversion per step.  Not part of the
 * reference. */
typedef struct gsvc_train_step_args {
    int num_points;
    float *xyz, *cholesky;
    const float *cholesky_bound;
    float *features, *rgb_w;
    int rgb_w_trainable;
    const float *background, *gt;
    unsigned img_height, img_width;
    int loss_kind, frame_index;
    float *const *adan_state;
    const double *adan_hparams;
    int adan_flags;
    float *loss, *render_out, *grads_out;
    void *workspace;
    size_t workspace_bytes;
    void *stream;
    /* GSVC_TRAIN_DETERMINISTIC only (else NULL / 0) */
    void *det_workspace;
    size_t det_workspace_bytes;
    long long det_capacity;
    /* loss_kind 2 only (else NULL / 0; see "Weighted Y/U/V loss" above) */
    const float *loss_yuv; /* host float[12]: M row-major (rows Y, U, V), then w_Y, w_U, w_V */
    int loss_chroma;       /* 0: 4:2:0, 1: 4:2:2, 2: 4:4:4 (the container's chroma codes) */
} gsvc_train_step_args;
int gsvc_train_step_sum_args(const gsvc_train_step_args *args);

/* The same render for a batch of ``frames`` frame models of one video (a
 * decoder's GOP: frame k of GSVC's gmodels_state_dict is its own model), one
 * call, two kernels over all frames: frame b's splats are
 * [frame_offsets[b], frame_offsets[b + 1]) of the concatenated inputs (host
 * and device copies of the int[frames + 1] offsets, offsets[0] = 0); its
 * image is out + b * 3*H*W (out [frames,3,H,W]); meta int[frames][2].
 * Images are bit-identical to per-frame gsvc_render_frame_sum calls.
 * Workspace sized by gsvc_render_frames_workspace_bytes, first
 * gsvc_render_frames_zeroed_bytes zero before the first call; call_index
 * alternates parity between calls on one workspace. */
size_t gsvc_render_frames_workspace_bytes(int frames, int num_points, unsigned img_height,
                                          unsigned img_width);
size_t gsvc_render_frames_zeroed_bytes(int frames, unsigned img_height, unsigned img_width);
int gsvc_render_frames_sum(int frames, const int *frame_offsets_host,
                           const int *frame_offsets_dev, const float *xyz, int xyz_tanh,
                           const float *cholesky, const float *cholesky_bound,
                           const float *features, const float *rgb_w, const float *opacity,
                           const float *background, unsigned img_height, unsigned img_width,
                           int call_index, int density_hint, int *meta, void *workspace,
                           size_t workspace_bytes, float *out, void *stream);

/* The same batch of frame models at another output size and window (a view;
 * not part of the reference): out [frames,3,out_h,out_w].  A frame model is a
 * function of position -- per 16x16 tile of the SOURCE grid, the tile's first
 * <= 256 entries in splat-id order -- which the native render samples at the
 * integer coordinates (j, i).  Source pixel j is the sample at the centre of
 * [j, j + 1) (half-pixel centres, as swscale and align_corners=False), so a
 * view of the window x0, y0, w, h (source pixels, fractions allowed,
 * 0 <= x0, w > 0, x0 + w <= W; rows alike) at out_h x out_w evaluates output
 * column j' at, in float64 and in this order,
 *     xd[j'] = x0 + ((2 j' + 1) w) / (2 out_w) - 0.5
 * with the entry list of the tile that owns source pixel
 *     p[j'] = min(max(floor(xd[j'] + 0.5), 0), W - 1),   tile p[j'] >> 4.
 * The four tables, per axis (columns; rows alike with y, h, out_h, H, tby):
 *     sample_x  float[out_w]   (float)xd[j']
 *     col_start int[tbx + 1]   the number of j' whose owner tile is below t:
 *                              p is monotone, so tile column t owns the output
 *                              columns [col_start[t], col_start[t + 1]), a
 *                              possibly empty range; the ranges partition
 *                              [0, out_w)
 * given as host and device copies (as frame_offsets): GSVC_ERR_ARG before any
 * launch unless col_start[0] = 0, col_start[tbx] = out_w and col_start is
 * non-decreasing (rows alike), every sample lies in [-1, W] x [-1, H], every
 * buffer is there and out_h, out_w >= 1.  The rule is exact where it matters:
 * the identity view has xd = j' (the native render's bits), an integer window
 * at scale 1 xd = x0 + j' (the native render's window), and an odd integer
 * upscale k puts output column k j + (k - 1) / 2 at x0 + j.  Other views
 * point-sample the trained function: no prefilter, so a downscale aliases
 * where splats are smaller than an output pixel (gsvc_render_frames_filtered
 * below adds a box prefilter).
 * Projection, workspace, zeroed bytes, call_index parity and meta are those of
 * gsvc_render_frames_sum at the source size img_height x img_width (one
 * workspace may serve both entries); density_hint is accepted and unused.
 * One composite wave per (frame, source tile) evaluates the tile's samples
 * with the rasterizer's op sequence at (sample_x[j'], sample_y[i']) and
 * writes the clamped planes. */
int gsvc_render_frames_resampled(int frames, const int *frame_offsets_host,
                                 const int *frame_offsets_dev, const float *xyz, int xyz_tanh,
                                 const float *cholesky, const float *cholesky_bound,
                                 const float *features, const float *rgb_w, const float *opacity,
                                 const float *background, unsigned img_height, unsigned img_width,
                                 int call_index, int density_hint, int *meta, void *workspace,
                                 size_t workspace_bytes, const float *sample_x_host,
                                 const float *sample_y_host, const int *col_start_host,
                                 const int *row_start_host, const float *sample_x_dev,
                                 const float *sample_y_dev, const int *col_start_dev,
                                 const int *row_start_dev, unsigned out_h, unsigned out_w,
                                 float *out, void *stream);

/* The same views with a box prefilter, reduced inside the composite (not part
 * of the reference): out [frames,3,out_h,out_w], every output pixel the mean
 * of ky x kx point samples, ky, kx >= 1 and ky kx <= 64.
 *
 * The rule.  The FINE view of a view (out_h, out_w, window) is the
 * point-sampled view of size (ky out_h, kx out_w) over the same window: the
 * sampling rule above with out_h, out_w replaced, nothing else.  The four
 * tables given here are the fine view's (sample_x float[kx out_w], col_start
 * partitioning [0, kx out_w); rows alike).  Output pixel (i', j') is the box
 * mean of the fine samples (ky i' + a, kx j' + b), 0 <= a < ky, 0 <= b < kx,
 * each evaluated with the entry list of ITS OWN owner tile and clamped to
 * [0, 1] as the fine view's image is.  (A pixel is not owned by one tile: a
 * splat that does not reach the tile of the pixel's centre can still cover a
 * sub-sample a few source pixels outside it.)  The summation order, float32
 * throughout, is part of the rule:
 *   - the pixel's sub-samples are split by owner tile into up to 2 x 2 parts,
 *         slot = 2 (tile row - tile row of sub-row ky i')
 *                + (tile column - tile column of sub-column kx j');
 *   - each part is summed in row-major (a, b) order, starting from +0.0f;
 *   - the parts are added in slot order;
 *   - the sum is divided by (float)(ky kx), correctly rounded.
 * A pixel inside one tile is therefore the plain row-major sum.  ky = kx = 1
 * is the point-sampled view, bit for bit.
 * Two tiles per axis: along an axis the tile of a pixel's last sub-sample is
 * the tile of its first one or the next (so every slot is 0..3; tiles are
 * counted from the first to the last, a skipped tile included).  A view that
 * breaks this -- more than about 16 source pixels per output pixel -- is
 * refused, decided from the start tables, not from the scale.
 *
 * parts: float[frames][4 slots][3][out_h][out_w], sized for the full output
 * (parts_bytes >= 48 frames out_h out_w; small, this is a downscale), scratch
 * of this call alone: the composite writes the part of every (pixel, slot)
 * whose pixel straddles a tile edge, a second kernel adds a straddler's parts
 * in slot order, divides and stores; it reads only slots written by this call,
 * so the buffer needs no initial value and carries nothing between calls.
 *
 * GSVC_ERR_ARG before any launch unless ky kx <= 64, the tables pass the
 * checks of gsvc_render_frames_resampled for ky out_h x kx out_w, the
 * two-tiles condition holds and parts is there and large enough.  Everything
 * else -- projection at the source size, workspace, zeroed bytes, call_index
 * parity, meta, density_hint -- is gsvc_render_frames_resampled's; one
 * workspace may serve all three batched entries in any order. */
int gsvc_render_frames_filtered(int frames, const int *frame_offsets_host,
                                const int *frame_offsets_dev, const float *xyz, int xyz_tanh,
                                const float *cholesky, const float *cholesky_bound,
                                const float *features, const float *rgb_w, const float *opacity,
                                const float *background, unsigned img_height, unsigned img_width,
                                int call_index, int density_hint, int *meta, void *workspace,
                                size_t workspace_bytes, const float *sample_x_host,
                                const float *sample_y_host, const int *col_start_host,
                                const int *row_start_host, const float *sample_x_dev,
                                const float *sample_y_dev, const int *col_start_dev,
                                const int *row_start_dev, unsigned ky, unsigned kx, unsigned out_h,
                                unsigned out_w, float *parts, size_t parts_bytes, float *out,
                                void *stream);

/* Replaces _C.rasterize_sum_backward (bindings.cu:706-779 -> backward.cu:696-862).
 * Gradients are written into one 64-byte record per splat,
 * grad_records [N,16] float: [0:2] v_xy, [2:5] v_conic, [5:8] v_colors,
 * [8] v_opacity, [9:16] unused (zeroed).  The Python layer returns strided
 * views of it.  v_output [H,W,3]; v_output_alpha, background and final_Ts are
 * accepted and unused, as in the reference sum kernel. */
int gsvc_rasterize_sum_backward(
    unsigned img_height, unsigned img_width, unsigned block_h, unsigned block_w,
    int num_points, const int *gaussian_ids_sorted, const int *tile_bins,
    const float *xys, const float *conics, const float *colors,
    const float *opacities, const float *background, const float *final_Ts,
    const int *final_idx, const float *v_output, const float *v_output_alpha,
    float *grad_records, void *stream);

/* The same backward with bitwise reproducible sums (the op path under
 * torch.use_deterministic_algorithms; not part of the reference, whose
 * backward.cu:843-859 adds with float atomics): each (splat, tile) sum is
 * stored to its own slot -- det_off[splat] + the tile's row-major index in the
 * splat's tile bbox, from xys and radii -- and every splat then adds its slots
 * in that order.  det_workspace of
 * gsvc_rasterize_sum_backward_det_workspace_bytes(num_points, det_capacity)
 * bytes; pairs past det_capacity fall back to the atomics.  pairs_out
 * (optional, device int): the (splat, tile) pair count, to size the capacity. */
size_t gsvc_rasterize_sum_backward_det_workspace_bytes(int num_points, long long det_capacity);
int gsvc_rasterize_sum_backward_det(
    unsigned img_height, unsigned img_width, unsigned block_h, unsigned block_w,
    int num_points, const int *gaussian_ids_sorted, const int *tile_bins,
    const float *xys, const float *conics, const float *colors,
    const float *opacities, const int *radii, const int *final_idx,
    const float *v_output, float *grad_records, void *det_workspace,
    size_t det_workspace_bytes, long long det_capacity, int *pairs_out, void *stream);

/* ---------------------------------------------------------------------------
 * Alpha-compositing rasterizer (rasterize.py; north_star's front-to-back path).
 * Replaces _C.rasterize_forward (bindings.cu:332-398 -> forward.cu:252-374). */
int gsvc_rasterize_forward(
    int tile_bounds_x, int tile_bounds_y, int tile_bounds_z,
    int block_x, int block_y, int block_z,
    unsigned img_width, unsigned img_height, unsigned img_depth,
    const int *gaussian_ids_sorted, const int *tile_bins,
    const float *xys, const float *conics, const float *colors,
    const float *opacities, const float *background,
    float *out_img, float *final_Ts, int *final_idx, void *stream);

/* Replaces _C.rasterize_backward (bindings.cu:631-704 -> backward.cu:138-315).
 * Same grad_records layout as gsvc_rasterize_sum_backward. */
int gsvc_rasterize_backward(
    unsigned img_height, unsigned img_width, unsigned block_h, unsigned block_w,
    int num_points, const int *gaussian_ids_sorted, const int *tile_bins,
    const float *xys, const float *conics, const float *colors,
    const float *opacities, const float *background, const float *final_Ts,
    const int *final_idx, const float *v_output, const float *v_output_alpha,
    float *grad_records, void *stream);

/* ---------------------------------------------------------------------------
 * Video input (utils.py:134-156 process_yuv_video + ToTensor,
 * train_video_Represent.py:204-207): one planar I420 frame (Y H*W bytes, then
 * U and V (H/2)*(W/2) each, device memory) to out [3,H,W] float RGB / 255 with
 * OpenCV's COLOR_YUV2RGB_I420 fixed-point BT.601 arithmetic.  H, W even. */
int gsvc_i420_to_rgb(const unsigned char *yuv, int height, int width, float *out, void *stream);

/* Video output (not in the reference, which writes no YUV; csrc/yuv_conv.hip, as
 * every conversion entry below): the inverse of the above for a batch.  rgb
 * [frames][3][H][W] fp32 (any values), out frames * (H*W*3/2) bytes: per frame
 * Y (H*W), U, V ((H/2)*(W/2) each).  Per channel
 * q = (int)(min(max(x, 0), 1) * 255 + 0.5) (NaN -> 0); Y = (269484 R + 528482 G
 * + 102760 B + (16 << 20) + (1 << 19)) >> 20; with Rs, Gs, Bs the sums of q over
 * a 2x2 block, U = (-155188 Rs - 305135 Gs + 460324 Bs + (128 << 22) + (1 << 21))
 * >> 22 and V = (460324 Rs - 385875 Gs - 74448 Bs + ...) >> 22 (BT.601 limited
 * range; int32; saturated to [0, 255]).
 * ref: NULL, or source I420 frames in out's layout; then sse[frames][3] (Y, U, V)
 * receives the exact integer sums of squared byte differences (the entry zeroes
 * sse on the stream first).  H, W even, > 0.  Any alignment: W % 8 == 0 with rgb
 * 16-byte and out / ref 8-byte aligned takes the vector kernel, everything else
 * the bytewise one; both write the same bytes.  GSVC_ERR_ARG before any launch
 * for frames <= 0, a size that is not positive and even, a missing buffer, ref
 * without sse, and a frame of more than 2^31 - 1 blocks of 256 chroma samples
 * (which no allocation can hold). */
int gsvc_rgb_to_i420(int frames, const float *rgb, int height, int width, unsigned char *out,
                     const unsigned char *ref, unsigned long long *sse, void *stream);

/* Pixel formats beyond the two entries above (csrc/yuv_conv.hip):
 * planar YUV 4:2:0 of 8, 10, 12 or 16 bits per sample, BT.601 or BT.709, limited
 * or full range.  Samples of more than 8 bits are 16-bit little-endian words with
 * the value in the low bits (yuv420p10le, ...12le, ...16le); planes Y, U, V.
 *
 * The legacy format {8, 0, 0} belongs to gsvc_i420_to_rgb / gsvc_rgb_to_i420,
 * which hold OpenCV's three-decimal constants; the two conversion entries below
 * use exact coefficients, differ from them by a level here and there, and so
 * REFUSE that one format (GSVC_ERR_ARG): one definition per format.
 *
 * With b the depth, s = b - 8, P = 2^b - 1; (Kr, Kb) = (0.299, 0.114) for BT.601,
 * (0.2126, 0.0722) for BT.709, Kg = 1 - Kr - Kb; limited range Yoff = 16 << s,
 * Yspan = 219 << s, Cspan = 224 << s, full range Yoff = 0, Yspan = Cspan = P;
 * Coff = 2^(b-1); fix(x) = floor(x * 2^20 + 0.5) in double:
 *   cY = fix(P/Yspan), cRV = fix(2(1-Kr) P/Cspan), cGU = fix(-2Kb(1-Kb)/Kg P/Cspan),
 *   cGV = fix(-2Kr(1-Kr)/Kg P/Cspan), cBU = fix(2(1-Kb) P/Cspan);
 *   yR = fix(Kr Yspan/P), yG = fix(Kg Yspan/P), yB = fix(Kb Yspan/P);
 *   uR = fix(-Kr/(2(1-Kb)) Cspan/P), uG = fix(-Kg/(2(1-Kb)) Cspan/P), uB = fix(Cspan/(2P));
 *   vR = fix(Cspan/(2P)), vG = fix(-Kg/(2(1-Kr)) Cspan/P), vB = fix(-Kb/(2(1-Kr)) Cspan/P). */
typedef struct {
    int bit_depth;  /* 8, 10, 12, 16 */
    int matrix;     /* 0 bt601, 1 bt709 */
    int full_range; /* 0 limited, 1 full */
} gsvc_yuv_format;

/* Host only, any of the 16 formats (the legacy one too: a query, not a
 * conversion): out = P, Yoff, Coff, bytes per sample, then the 14 coefficients
 * in the order above. */
int gsvc_yuv_format_table(const gsvc_yuv_format *fmt, long long out[18]);

/* yuv: frames * (H*W*3/2) samples (device) -> out [frames][3][H][W] fp32.  Per
 * pixel, with the chroma sample of its 2x2 block: y = max(0, Y - Yoff) cY + 2^19,
 * u = U - Coff, v = V - Coff; R = clamp((y + cRV v) >> 20, 0, P), G = clamp((y +
 * cGV v + cGU u) >> 20, 0, P), B = clamp((y + cBU u) >> 20, 0, P) (arithmetic
 * shift; 64-bit above 8 bits); out = (float)X / (float)P.  A 16-bit sample above
 * P is taken as it is.  H, W even, > 0; a 16-bit buffer at an odd address is an
 * argument error. */
int gsvc_yuv420_to_rgb(int frames, const void *yuv, int height, int width,
                       const gsvc_yuv_format *fmt, float *out, void *stream);

/* The inverse, as gsvc_rgb_to_i420: q = (int)(min(max(x, 0), 1) * (float)P + 0.5f)
 * (NaN -> 0); Y = clamp((yR R + yG G + yB B + (Yoff << 20) + 2^19) >> 20, 0, P);
 * with Rs, Gs, Bs the sums of q over a 2x2 block, U = clamp((uR Rs + uG Gs + uB Bs
 * + (Coff << 22) + 2^21) >> 22, 0, P), V likewise.  out: frames * (H*W*3/2)
 * samples.  ref: NULL, or source frames in out's layout; then sse[frames][3]
 * receives the exact sums of squared sample differences (zeroed on the stream by
 * the entry).  W % 8 == 0 with rgb, out and ref 16-byte aligned takes one lane per
 * 2 rows x 8 columns, everything else one lane per 2x2 block; same bytes. */
int gsvc_rgb_to_yuv420(int frames, const float *rgb, int height, int width,
                       const gsvc_yuv_format *fmt, void *out, const void *ref,
                       unsigned long long *sse, void *stream);

/* Chroma layouts beyond planar 4:2:0 (csrc/yuv_conv.hip), for
 * every gsvc_yuv_format: chroma = 420, 422 or 444; semi_planar = 0: planes Y, U,
 * V; 1: plane Y, then one plane of interleaved U, V pairs, U first (NV12 / NV16 /
 * NV24).  Samples per frame: Y H*W; U and V each (H/2)*(W/2) at 420 (H, W even),
 * H*(W/2) at 422 (W even), H*W at 444 (any H, W > 0).  Above 8 bits a planar word
 * holds the value in its low bits, a semi-planar word in its high bits (the P010
 * family: word = value << (16 - b); read as word >> (16 - b), the low bits
 * ignored; written with the low bits zero).
 *
 * The formulas are those of the two entries above with the chroma block
 * generalised: pixel (i, j) takes the chroma sample at (i >> 1, j >> 1), (i,
 * j >> 1) or (i, j); on output Rs, Gs, Bs are the sums of q over the sample's
 * block of n = 4, 2 or 1 pixels and U = clamp((uR Rs + uG Gs + uB Bs + (Coff <<
 * sh) + 2^(sh-1)) >> sh, 0, P) with sh = 20 + log2 n, V likewise.  Coefficients:
 * gsvc_yuv_format_table's, except for the legacy triple {8, 0, 0}, which takes
 * the constants of gsvc_i420_to_rgb / gsvc_rgb_to_i420 (one definition per
 * colour triple: NV12 out is a byte permutation of gsvc_rgb_to_i420's I420).
 *
 * Planar 4:2:0 (chroma 420, semi_planar 0) belongs to the four entries above and
 * is REFUSED here (GSVC_ERR_ARG).  GSVC_ERR_ARG before any launch also for: a
 * chroma other than the three, a bad format, frames <= 0, a size that breaks the
 * chroma's constraint, a missing buffer, ref without sse, a 16-bit buffer at an
 * odd address.  W % 8 == 0 with every buffer 16-byte aligned takes one lane per
 * 2 (420) or 1 rows x 8 columns, everything else one lane per chroma block; same
 * bytes.
 *
 * yuv: frames of the layout (device) -> out [frames][3][H][W] fp32. */
int gsvc_yuv_to_rgb(int frames, const void *yuv, int height, int width, const gsvc_yuv_format *fmt,
                    int chroma, int semi_planar, float *out, void *stream);

/* rgb [frames][3][H][W] fp32 (any values) -> out: frames of the layout.  ref: NULL,
 * or source frames in out's layout (U and V taken apart from an interleaved
 * plane, the P010 family's low bits ignored); then sse[frames][3] (Y, U, V)
 * receives the exact sums of squared sample differences (zeroed on the stream by
 * the entry). */
int gsvc_rgb_to_yuv(int frames, const float *rgb, int height, int width, const gsvc_yuv_format *fmt,
                    int chroma, int semi_planar, void *out, const void *ref,
                    unsigned long long *sse, void *stream);

/* ---- SSIM / MS-SSIM (the loss_fn SSIM variants, utils.py:29-40, and the
 * per-frame MS-SSIM metric, train_video_Represent.py:145), restating
 * pytorch_msssim's ssim() / ms_ssim() (_ssim, gaussian_filter, avg-pool
 * pyramid).  X, Y: [batch*channels][H][W] fp32 device planes.  levels = 1:
 * ssim() (or, with flag bit2, ms_ssim() with one weight); levels > 1: ms_ssim()
 * with `weights` (host, levels values).
 * flags: bit0 size_average (out[1]; else out[batch] = mean over channels),
 * bit1 nonnegative_ssim (ssim() only), bit2 the multi-scale formula
 * prod_i relu(term_i)^weights[i] (implied by levels > 1; with levels = 1 it is
 * ms_ssim() with a single weight, relu(ssim)^weights[0], where levels = 1
 * without it is ssim()).  C1 = (K1 data_range)^2, C2 = (K2 data_range)^2.
 * The forward leaves in `ws` what the backward needs (pooled levels, upstream
 * factors): pass the same workspace to the backward.  win_size odd, <= 11. */
size_t gsvc_ssim_workspace_bytes(int planes, int height, int width, int win_size, int levels);
int gsvc_ssim_forward(int batch, int channels, int height, int width, const float *X,
                      const float *Y, int win_size, float win_sigma, float C1, float C2,
                      int levels, const double *weights, int flags, float *out, void *ws,
                      size_t ws_bytes, void *stream);
/* d(out)/dX and/or d(out)/dY (either may be NULL) times grad_out (device,
 * out's shape).  `ws`: the forward's workspace; `scratch`: a temporary of
 * gsvc_ssim_backward_scratch_bytes (the coefficient maps and coarse-level
 * gradients; free after the call). */
size_t gsvc_ssim_backward_scratch_bytes(int planes, int height, int width, int win_size,
                                        int levels);
int gsvc_ssim_backward(int batch, int channels, int height, int width, const float *X,
                       const float *Y, int win_size, float win_sigma, float C1, float C2,
                       int levels, int flags, const float *grad_out, float *dX, float *dY,
                       void *ws, size_t ws_bytes, void *scratch, size_t scratch_bytes,
                       void *stream);

/* ---------------------------------------------------------------------------
 * Compression stage (GaussianSplats_Compress.py forward_quantize over
 * quantize.py; DESIGN.md section 13 has the op orders bit-exactness rests on).
 *
 * Quantized parameters of one frame model, all fp32 contiguous:
 *   xq [N,2] = float(half(xyz)) (+ p_xyz), before tanh;
 *   Lq [N,3] = ((q * scale + beta) + cholesky_bound) (+ p_cholesky) with
 *              q = round_half_even(clamp((cholesky - beta) / scale, 0, 63));
 *   cq [N,3] = (e0 + e1) (+ p_features): the nearest codeword of
 *              codebooks[0] to f and of codebooks[1] to f - e0 (squared
 *              distance summed over d ascending, lowest index of equal ones);
 *   codes_chol [N,3], codes_rgb [N,2]: uint8.
 * scale, beta, cholesky_bound: [3]; codebooks: [2][8][3].  p_xyz, p_cholesky,
 * p_features: the previous frame's parameters of a delta frame, all three or
 * all NULL.  commit_sums (optional, [2]): per stage, the sum over splats of
 * the squared distance to the chosen codeword, reduced in a fixed order
 * through `workspace` (gsvc_quant_workspace_bytes; only read when commit_sums
 * is set).  N = 0 launches nothing. */
size_t gsvc_quant_workspace_bytes(int num_points);
int gsvc_quant_params_forward(
    int num_points, const float *xyz, const float *cholesky, const float *features,
    const float *scale, const float *beta, const float *codebooks, const float *cholesky_bound,
    const float *p_xyz, const float *p_cholesky, const float *p_features, float *xq, float *Lq,
    float *cq, unsigned char *codes_chol, unsigned char *codes_rgb, float *commit_sums,
    void *workspace, size_t workspace_bytes, void *stream);

/* Straight-through backward of the above.  With raw = (cholesky - beta) / scale,
 * mask = (0 <= raw <= 63), q = round(clamp(raw)):
 *   v_xyz = v_xq;  v_cholesky = v_Lq * mask;
 *   v_scale[k] = sum_n v_Lq * (q - mask * raw);  v_beta[k] = sum_n v_Lq * (1 - mask);
 *   v_features = 2 * v_cq + (v_commit[0] * 2 (f - e0) + v_commit[1] * 2 ((f - e0) - e1)).
 * v_commit ([2], optional): the gradients of commit_sums; NULL drops the term
 * (features, codebooks and codes_rgb are then not read).  codes_rgb: the
 * forward's.  v_scale, v_beta ([3] each) are reduced in a fixed order, no
 * float atomics: equal inputs give equal bits. */
int gsvc_quant_params_backward(
    int num_points, const float *cholesky, const float *features, const float *scale,
    const float *beta, const float *codebooks, const unsigned char *codes_rgb, const float *v_xq,
    const float *v_Lq, const float *v_cq, const float *v_commit, float *v_xyz, float *v_cholesky,
    float *v_features, float *v_scale, float *v_beta, void *workspace, size_t workspace_bytes,
    void *stream);

/* The packed stream of one frame, little-endian, GSVC_STREAM_HEADER_BYTES +
 * GSVC_STREAM_SPLAT_BYTES * N bytes:
 *   header: u32 magic, u32 version, i32 N, u32 H, u32 W, u32 flags (bit 0: a
 *           delta frame), f32 scale[3], beta[3], codebooks[48]; zero to the end;
 *   plane A, N x 4 bytes: half(x), half(y);
 *   plane B, N x 3 bytes: c0 | c1 << 6 | c2 << 12 | i0 << 18 | i1 << 21.
 * gsvc_pack_splats writes the two planes (7 N bytes at `planes`) from xyz and
 * the forward's codes; the caller writes the header. */
#define GSVC_STREAM_MAGIC 0x51565347u /* "GSVQ" */
#define GSVC_STREAM_VERSION 1
#define GSVC_STREAM_HEADER_BYTES 256
#define GSVC_STREAM_SPLAT_BYTES 7
int gsvc_pack_splats(int num_points, const float *xyz, const unsigned char *codes_chol,
                     const unsigned char *codes_rgb, unsigned char *planes, void *stream);

/* Decodes num_frames concatenated frame streams in one launch to xq, Lq, cq
 * (frame f's splats follow frame f-1's; the bits of the forward entry above
 * for the same half / codes / tables).  stream_host: the bytes in host memory,
 * validated before any launch (magic, version, N >= 0, each frame's length
 * against frame_offsets [num_frames + 1] host byte offsets, one H x W);
 * stream_dev: the same bytes in device memory, which the kernel reads.  A
 * delta frame adds the decoded pre-activation parameters of the frame before
 * it (its first N splats; N may not exceed that frame's count): frame f-1 of
 * this call, or for frame 0 prev_xyz / prev_cholesky / prev_features
 * [prev_points] -- xq, Lpre and cq of the previous call's last frame.  A
 * delta frame 0 with prev_points = 0 is an error.  Lpre (optional, [total,3]):
 * Lq without cholesky_bound.  out_capacity: splats the outputs hold. */
int gsvc_unpack_splats(int num_frames, const unsigned char *stream_host,
                       const long long *frame_offsets, const unsigned char *stream_dev,
                       const float *cholesky_bound, const float *prev_xyz,
                       const float *prev_cholesky, const float *prev_features, int prev_points,
                       float *xq, float *Lq, float *cq, float *Lpre, long long out_capacity,
                       void *stream);

/* The entropy-coded stream of one frame (version 2), a lossless transcoding of
 * the version-1 stream above, little-endian:
 *   bytes 0-239:   the version-1 header with version = GSVC_STREAM_VERSION_CODED;
 *   bytes 240-255: u16 S (splats per segment, 1..4096), u16 prob_bits (12),
 *                  u32 n_seg = ceil(N / S), u32 payload_bytes, u32 zero;
 *   tables, 1440 bytes: for the channels c0, c1, c2 (alphabet 64 each), i0, i1
 *                  (8 each), high byte of half(x), of half(y) (256 each) the
 *                  u16 frequencies of the symbols; each channel sums to 4096;
 *   2 N bytes:     per splat the low byte of half(x), of half(y);
 *   directory:     n_seg + 1 u32 offsets into the payload: 0 first,
 *                  payload_bytes last, even, each segment at least 4 bytes;
 *   payload:       per segment of S splats a u32 rANS state, then the u16 words
 *                  in the order the decoder consumes them (32-bit state,
 *                  L = 2^16, splat-major, the seven channels per splat in the
 *                  order above).
 * The three entries below take frames of either version in one list and, like
 * gsvc_unpack_splats, validate the host copy before any launch: everything
 * above that needs no decoding (not a segment's final state, which only the
 * host decoder gsvc_amd.ans.entropy_expand checks). */
#define GSVC_STREAM_VERSION_CODED 2

/* expanded_offsets [num_frames + 1]: the byte offsets the frames have once
 * every one is expanded to version 1 (256 + 7 N bytes each). */
int gsvc_stream_expanded_bytes(int num_frames, const unsigned char *stream_host,
                               const long long *frame_offsets, long long *expanded_offsets);

/* Transcodes the frames at stream_dev to version-1 bytes at expanded_dev
 * (expanded_capacity bytes; GSVC_ERR_WORKSPACE when they do not fit): one
 * kernel, one lane per frame and segment; a version-1 frame is copied.  The
 * kernel re-derives and clamps everything it reads from the device copy, so a
 * device copy that differs from the validated host copy decodes to other
 * bytes, not out of bounds. */
int gsvc_expand_stream(int num_frames, const unsigned char *stream_host,
                       const long long *frame_offsets, const unsigned char *stream_dev,
                       unsigned char *expanded_dev, size_t expanded_capacity, void *stream);

/* gsvc_unpack_splats for frames of either version: expands the list into
 * workspace (workspace_bytes >= expanded_offsets[num_frames]; not used when
 * every frame is version 1), then runs gsvc_unpack_splats' frame walk on it. */
int gsvc_unpack_stream(int num_frames, const unsigned char *stream_host,
                       const long long *frame_offsets, const unsigned char *stream_dev,
                       const float *cholesky_bound, const float *prev_xyz,
                       const float *prev_cholesky, const float *prev_features, int prev_points,
                       float *xq, float *Lq, float *cq, float *Lpre, long long out_capacity,
                       void *workspace, size_t workspace_bytes, void *stream);

/* The encoder of the version-2 stream: for every frame exactly the bytes
 * gsvc_amd.ans.entropy_code(stream_v1, segment) gives (gsvc_amd/ans.py is the
 * host statement both entries below mirror: its _symbols, normalise, coder and
 * layout; DESIGN.md 13b "Encoder").  num_points [num_frames] are the frames'
 * splat counts in host memory; everything is sized by them, never by a header
 * in device memory.
 *
 * gsvc_encode_stream_bytes mirrors ans.coded_length at the worst-case payload
 * (every symbol emits a word): coded_offsets [num_frames + 1] are the byte
 * offsets of the frames' slots in the output buffer, each slot 256 + 1440 +
 * 2 N + 4 (n_seg + 1) + 4 n_seg + 14 N bytes rounded up to a multiple of 4;
 * *workspace_bytes is what gsvc_encode_stream needs.  GSVC_ERR_ARG for a
 * segment outside 1..4096, a negative count, or a worst-case payload beyond
 * the format's u32 offsets. */
int gsvc_encode_stream_bytes(int num_frames, const int *num_points, int segment,
                             long long *coded_offsets, size_t *workspace_bytes);

/* Codes the num_frames concatenated version-1 frames at frames_dev (256 + 7 N
 * bytes each, at any byte offsets) as ans.entropy_code does: frame f's coded
 * bytes start at coded_dev + coded_offsets[f] and coded_bytes_dev[f] (device,
 * 64-bit) receives their length; the bytes between that length and the next
 * slot are unspecified.  Histograms, ans.normalise, the coder, the directory
 * scan and the assembly of the frame all run on the device, in integers, up to
 * 32 frames per launch; equal inputs give equal bytes.  The output header
 * carries the host's N.  The workspace is 16-byte aligned.  Argument errors as
 * above; GSVC_ERR_WORKSPACE, before any launch, when coded_capacity is below
 * coded_offsets[num_frames] or workspace_bytes below the query's figure. */
int gsvc_encode_stream(int num_frames, const int *num_points, const unsigned char *frames_dev,
                       int segment, unsigned char *coded_dev, size_t coded_capacity,
                       long long *coded_bytes_dev, void *workspace, size_t workspace_bytes,
                       void *stream);

/* ---------------------------------------------------------------------------
 * Fused quantized training step of the compression stage: one
 * train_iter_quantize (GaussianSplats_Compress.py:86-98, 181-193) with the L2
 * or L1 loss and Adan, one call, no host sync, no allocation.  On ``stream``
 * it enqueues, in order:
 *   1. the quantizer forward (gsvc_quant_params_forward's kernel with its
 *      commitment sums) into xq, Lq, cq and the code buffers of ``workspace``;
 *   2. gsvc_train_step_sum_args in gradients-only mode on (xq, Lq, cq): tanh,
 *      projection, binning, forward, clamp, loss, backward; no cholesky_bound
 *      (Lq holds it), no rgb_w; its gradient records [N,9] go to the
 *      workspace, the image bits of gsvc_render_frame_sum to render_out;
 *   3. the per-splat kernel: gsvc_quant_params_backward's op sequence with
 *      v_commit[0] = v_commit[1] = (float)(commitment_weight / (3 N)) and the
 *      PRE-step codebooks, the Adan update (gsvc_adan_step's op sequence) of
 *      xyz, cholesky and features in place, block partials of v_scale, v_beta
 *      (gsvc_quant_params_backward's reduction: the same bits) and of the
 *      codebooks' member counts and sums -- stage 0: the features f under
 *      i0, stage 1: f - e0 (pre-step e0) under i1, both from the PRE-update
 *      features, as ResidualVQ8.ema_update sees them in the forward; these
 *      are added in double: each wave's 64 members in splat order, pass after
 *      pass of the grid's stride loop, then the block's four waves in order;
 *   4. a one-workgroup kernel: the partials in block order (the member sums
 *      in double, rounded to float once), the Adan update of scale and beta,
 *      and per stage, with the float decay d and 1 - d,
 *        cluster_size = fma(1 - d, counts, cluster_size * d)   (embed_avg alike)
 *        total = sum of cluster_size in index order
 *        smoothed = (cluster_size + eps) / (total + 8 eps) * total
 *        codebooks = embed_avg / smoothed
 *      and loss[0..3] = {mean squared error, mean absolute error, commitment
 *      sum of stage 0, of stage 1} (device or pinned host memory; read it
 *      after gsvc_stream_sync).  The step's loss is loss[loss_kind] +
 *      commitment_weight * (loss[2] + loss[3]) / (3 N); with loss_kind 2
 *      (the weighted Y/U/V loss of gsvc_train_step_sum_args, from loss_yuv
 *      and loss_chroma) loss[1] holds that loss and takes loss[loss_kind]'s
 *      place.
 * No float atomics anywhere in 1, 3 and 4: equal inputs give equal bits (step
 * 2 with GSVC_TRAIN_DETERMINISTIC in ``flags``, which needs det_workspace).
 * adan_state: host array of 20 device pointers, per parameter (xyz, cholesky,
 * features, scale, beta) its {exp_avg, exp_avg_sq, exp_avg_diff,
 * neg_pre_grad}; adan_hparams: the ten of gsvc_train_step_sum.  flags: bit 0
 * no_prox; bit 1 + q: parameter q takes its first step;
 * GSVC_TRAIN_DETERMINISTIC.  p_xyz, p_cholesky, p_features: all three (a delta
 * frame) or all NULL.  train_workspace (gsvc_train_step_workspace_bytes,
 * zeroed and with frame_index's parity as for gsvc_train_step_sum) and
 * det_workspace belong to step 2.  grads_out (test hook, [8 N + 6]): when
 * non-NULL nothing is updated -- no parameter, state or codebook byte -- and
 * the gradients go there: v_xyz [N,2], v_cholesky [N,3], v_features [N,3],
 * v_scale [3], v_beta [3].  Everything is validated before the first launch;
 * num_points < 1 is an argument error; a capturing stream is refused
 * (GSVC_ERR_CAPTURE) as by gsvc_train_step_sum.  Not part of the reference. */
typedef struct gsvc_quant_train_args {
    int num_points;
    float *xyz, *cholesky, *features;             /* [N,2], [N,3], [N,3] */
    float *scale, *beta;                          /* [3] each */
    float *codebooks, *cluster_size, *embed_avg;  /* [2,8,3], [2,8], [2,8,3] */
    const float *cholesky_bound;                  /* [3] */
    const float *p_xyz, *p_cholesky, *p_features;
    const float *background, *gt;
    unsigned img_height, img_width;
    int loss_kind, frame_index;
    float *const *adan_state;
    const double *adan_hparams;
    int flags;
    double decay, eps, commitment_weight;
    float *loss, *render_out, *grads_out;
    void *workspace;
    size_t workspace_bytes;
    void *train_workspace;
    size_t train_workspace_bytes;
    void *det_workspace;
    size_t det_workspace_bytes;
    long long det_capacity;
    void *stream;
    /* loss_kind 2 only (else NULL / 0): gsvc_train_step_args' fields of the same names */
    const float *loss_yuv;
    int loss_chroma;
} gsvc_quant_train_args;
size_t gsvc_quant_train_workspace_bytes(int num_points);
int gsvc_quant_train_step(const gsvc_quant_train_args *args);
/* Steps 3 and 4 alone, on caller-given gradient records (grad_records [N,9] =
 * {d_xq 2, d_Lq 3, d_cq 3, unused}) and codes_rgb [N,2] (the forward's): the
 * render fields of ``args`` (background, gt, sizes, loss_kind, frame_index,
 * render_out, train / det workspace) are not read; ``loss`` is optional and
 * receives {0, 0, commit_sums[0], commit_sums[1]} (commit_sums optional,
 * device memory; zeros without). */
int gsvc_quant_adan_step(const gsvc_quant_train_args *args, const float *grad_records,
                         const unsigned char *codes_rgb, const float *commit_sums);

/* ``iterations`` (K >= 1) fused quantized training steps in one call, with no
 * host round trip in between, and the reference's "best state"
 * (train_video_Compress.py:89-102) kept on the device.  On step->stream the
 * call enqueues, for i = 0 .. K-1, exactly the launches of
 * gsvc_quant_train_step(step) with
 *   adan_hparams = run->adan_hparams + 10 i   (host array [K][10]),
 *   flags        = run->flags[i]              (host array [K]: no_prox, the
 *                  first-step bits; GSVC_TRAIN_DETERMINISTIC must be equal in
 *                  all K entries),
 *   frame_index  = step->frame_index + i      (the train workspace's parity),
 *   loss         = run->loss_log + 4 i        ([K][4], device or coherent host
 *                  memory; read it after gsvc_stream_sync).
 * step's own adan_hparams, flags and loss are not read.  step->grads_out must
 * be NULL: a run has no test-hook mode.
 *
 * The best-state block is best_mse, best_iter and the eight snapshot buffers
 * best_xyz [N,2], best_cholesky [N,3], best_features [N,3], best_scale [3],
 * best_beta [3], best_codebooks [2,8,3], best_cluster_size [2,8],
 * best_embed_avg [2,8,3] (device memory, 4-byte aligned, not overlapping the
 * step's tensors): every pointer set, or every pointer NULL -- they go
 * together.  When it is set, the keep-best kernel follows each iteration's
 * launches: with mse the float that loss_log[4 i] receives, and only when
 * mse < *best_mse (strict: the first of equal values stays; a NaN never
 * takes), it copies the eight tensors AS THE ITERATION LEFT THEM (after the
 * update) into the snapshot and sets *best_mse = mse, *best_iter = iter_base +
 * i.  This is the reference's rule: the PSNR of iteration i belongs to the
 * state before its update, the state saved is the one after it, and mse < best
 * is psnr > best_psnr for psnr = 10 log10(1 / mse).  *best_mse (start it at
 * +inf) and *best_iter (start it at -1) carry from call to call; iter_base is
 * the global index of this call's iteration 0.  Every workgroup of the kernel
 * decides from the same (mse, *best_mse): the two words are written by the
 * workgroup that arrives last at a ticket in ``workspace`` (zeroed by one
 * small launch at the head of the call).  Without the block nothing beyond the
 * K steps is enqueued.
 *
 * Everything -- the step's arguments as by gsvc_quant_train_step, the run's
 * own, all K flag words -- is validated before the first launch; a capturing
 * stream is refused (GSVC_ERR_CAPTURE).  A launch error at iteration i returns
 * at once, with the iteration in gsvc_last_error(); the iterations before it
 * stay enqueued.  Not part of the reference. */
typedef struct gsvc_quant_train_run_args {
    const gsvc_quant_train_args *step;
    int iterations;
    const double *adan_hparams;
    const int *flags;
    float *loss_log;
    float *best_mse;
    int *best_iter;
    int iter_base;
    float *best_xyz, *best_cholesky, *best_features;
    float *best_scale, *best_beta;
    float *best_codebooks, *best_cluster_size, *best_embed_avg;
} gsvc_quant_train_run_args;
int gsvc_quant_train_run(const gsvc_quant_train_run_args *run);

#ifdef __cplusplus
}
#endif

#endif /* GSVC_AMD_H */
