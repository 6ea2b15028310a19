// Fused quantized training step of the compression stage (gfx950): one C call
// per train_iter_quantize (GaussianSplats_Compress.py:86-98, 181-193).
//
// gsvc_quant_train_step enqueues the quantizer forward (quant.hip's kernel),
// gsvc_train_step_sum_args in gradients-only mode on its outputs (train.hip,
// unchanged: tanh, projection, binning, forward, loss, backward) and the two
// kernels of this file, which are the quantizer-side half of the step
// (DESIGN.md §13c):
//
//   quant_train_splat_kernel   one splat per lane, a grid of at most
//       kQuantMaxBlocks blocks striding over N.  The straight-through backward
//       (quant_dev.h quant_backward_splat: gsvc_quant_params_backward's op
//       sequence) on the render step's gradient record, the Adan update
//       (adan.h adan_update: gsvc_adan_step's) of the splat's 8 elements in
//       place, the block partial of v_scale / v_beta (quant_dev.h
//       block_partial: the bits of gsvc_quant_params_backward), and the block
//       partial of the codebooks' member counts and sums from the PRE-update
//       features and PRE-step codebooks.
//   quant_train_finish_kernel  one workgroup: the partials in block order,
//       Adan on scale and beta, the codebooks' moving average, the loss words.
//
// Reductions have a fixed order and no float atomics.  The 64 member values
// (2 stages x 8 codewords x {count, 3-vector sum}): every lane leaves its
// splat's (i0, i1, f, f - e0) in LDS; lane t of the block owns value
// (stage (t >> 5) & 1, codeword (t >> 2) & 7, component t & 3) over the
// members its wave's 64 lanes left and adds the matching ones in lane order,
// pass after pass of the stride loop, in DOUBLE; the block's partial is the
// four waves' sums added in wave order; the finish kernel adds the blocks'
// doubles in block order and rounds to float once.  (Counts are integers,
// exact either way; the sums come out within half an ulp of the exact sum,
// which is what holds embed_avg and the codebooks to the float64
// restatement's bar.)
#include "adan.h"
#include "frame.h"
#include "quant_dev.h"

namespace gsvc {

constexpr int kEmaValues = kStages * kCodewords * 4;  // 64: one lane of every wave each
static_assert(kEmaValues == 64, "a wave's lanes own the member values");
constexpr int kMemberRow = kQuantBlock + 1;  // padded: the 6 rows a wave reads sit on 6 banks

struct QuantTrainSplatArgs {
    int n, update;
    float *xyz, *chol, *feat;
    const float *scale, *beta, *cb;
    const unsigned char *codes_rgb;
    const float *rec;  // [N,9] = d_xq 2, d_Lq 3, d_cq 3, unused
    float vc;          // gradient of either commitment sum
    float *state[3][4];
    int first[3];
    AdanScalars S;
    float *grads_out;  // update == 0: v_xyz [N,2], v_cholesky [N,3], v_features [N,3]
    float *partials;   // [blocks, kQuantSums]
    double *epart;     // [blocks, kEmaValues]
};

__global__ __launch_bounds__(kQuantBlock) void quant_train_splat_kernel(QuantTrainSplatArgs A) {
    __shared__ int s_code[kQuantBlock];          // i0 | i1 << 3; -1: no splat
    __shared__ float s_val[6][kMemberRow];       // f (3), f - e0 (3)
    __shared__ double s_acc[kQuantBlock / 64][kEmaValues];
    const float scale[3] = {A.scale[0], A.scale[1], A.scale[2]};
    const float beta[3] = {A.beta[0], A.beta[1], A.beta[2]};
    const int t = threadIdx.x;
    const bool upd = A.update != 0;
    // the member value this lane owns, over its wave's 64 members
    const int es = (t >> 5) & 1, ej = (t >> 2) & 7, ec = t & 3;
    const int erow = ec == 0 ? 0 : 3 * es + ec - 1;
    double acc = 0.0;
    float sums[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};  // v_scale[3], v_beta[3]
    // (the loop bound is the block's, so every lane reaches the barriers)
    for (long long base = (long long)blockIdx.x * kQuantBlock; base < A.n;
         base += (long long)gridDim.x * kQuantBlock) {
        const long long i = base + t;
        int code = -1;
        float fv[3] = {0.0f, 0.0f, 0.0f}, r1[3] = {0.0f, 0.0f, 0.0f};
        if (i < A.n) {
            // every operand up front: one round trip per lane
            float p[8], rec[8];
            ld_row<2>(A.xyz, i, p);
            ld_row<3>(A.chol, i, p + 2);
            ld_row<3>(A.feat, i, p + 5);
#pragma unroll
            for (int e = 0; e < 8; ++e) rec[e] = A.rec[9 * i + e];
            const int i0 = A.codes_rgb[2 * i] & (kCodewords - 1);
            const int i1 = A.codes_rgb[2 * i + 1] & (kCodewords - 1);
            AdanRows<2> sx;
            AdanRows<3> sc, sf;
            if (upd) {
                adan_rows_load(sx, A.state[0], i);
                adan_rows_load(sc, A.state[1], i);
                adan_rows_load(sf, A.state[2], i);
            }
            fv[0] = p[5], fv[1] = p[6], fv[2] = p[7];
            code = i0 | (i1 << 3);
#pragma unroll
            for (int k = 0; k < 3; ++k) r1[k] = fv[k] - A.cb[3 * i0 + k];
            // the quantizer's backward: g = {v_xyz 2, v_cholesky 3, v_features 3}
            float g[8];
            g[0] = rec[0];
            g[1] = rec[1];
            quant_backward_splat(p + 2, rec + 2, rec + 5, scale, beta, true, fv, A.cb, i0, i1, A.vc,
                                 A.vc, g + 2, g + 5, sums);
            if (upd) {
                adan_rows_step(A.S, A.first[0], sx, p, g);
                adan_rows_step(A.S, A.first[1], sc, p + 2, g + 2);
                adan_rows_step(A.S, A.first[2], sf, p + 5, g + 5);
                st_row<2>(A.xyz, i, p);
                adan_rows_store(A.state[0], i, sx);
                st_row<3>(A.chol, i, p + 2);
                adan_rows_store(A.state[1], i, sc);
                st_row<3>(A.feat, i, p + 5);
                adan_rows_store(A.state[2], i, sf);
            } else {
                st_row<2>(A.grads_out, i, g);
                st_row<3>(A.grads_out + 2 * (size_t)A.n, i, g + 2);
                st_row<3>(A.grads_out + 5 * (size_t)A.n, i, g + 5);
            }
        }
        if (upd) {  // (uniform over the grid)
            // the block's members of this pass, then the owners add theirs in lane order
            __syncthreads();  // the previous pass's owners have read
            s_code[t] = code;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                s_val[k][t] = fv[k];
                s_val[3 + k][t] = r1[k];
            }
            __syncthreads();
            const int l0 = t & ~63;
#pragma unroll 8
            for (int l = l0; l < l0 + 64; ++l) {
                const int c = s_code[l];
                const float val = s_val[erow][l];
                if (c >= 0 && ((c >> (3 * es)) & (kCodewords - 1)) == ej)
                    acc += ec == 0 ? 1.0 : (double)val;
            }
        }
    }
    block_partial(sums, A.partials);
    if (upd) {
        s_acc[t >> 6][t & 63] = acc;
        __syncthreads();
        if (t < kEmaValues)
            A.epart[(size_t)blockIdx.x * kEmaValues + t] =
                ((s_acc[0][t] + s_acc[1][t]) + s_acc[2][t]) + s_acc[3][t];
    }
}

struct QuantTrainFinishArgs {
    int nblocks, update;
    const float *partials;
    const double *epart;
    float *scale, *beta;
    float *state[2][4];
    int first[2];
    AdanScalars S;
    float *cb, *cluster, *embed;
    float decay, one_m_decay, eps, eps_all;  // eps_all = (float)(kCodewords * eps)
    const float *render_loss;  // {mse, mae} or null
    const float *commit_sums;  // [2] or null
    float *loss;               // 4 words or null
    float *grads_tail;         // update == 0: v_scale [3], v_beta [3]
};

__global__ __launch_bounds__(kQuantBlock) void quant_train_finish_kernel(QuantTrainFinishArgs A) {
    __shared__ float s_ema[kEmaValues];               // (stage, codeword, {count, sum 3})
    __shared__ float s_cluster[kStages * kCodewords]; // the updated cluster sizes
    const int t = threadIdx.x;
    const bool upd = A.update != 0;
    if (t < 6) {
        // v_scale[3], v_beta[3]: quant_combine_kernel's order
        const float s = sum_block_order(A.partials + t, A.nblocks, kQuantSums);
        if (upd) {
            const int q = t / 3, k = t - 3 * q;
            float *par = q == 0 ? A.scale : A.beta;
            float m = A.state[q][0][k], v = A.state[q][1][k], df = A.state[q][2][k];
            float npg = A.state[q][3][k];
            if (A.first[q]) npg = -(s * A.S.clip);
            par[k] = adan_update(A.S, par[k], s, m, v, df, npg);
            A.state[q][0][k] = m;
            A.state[q][1][k] = v;
            A.state[q][2][k] = df;
            A.state[q][3][k] = npg;
        } else {
            A.grads_tail[t] = s;
        }
    } else if (t >= 64 && t < 64 + kEmaValues && upd) {
        // the member counts and sums: the blocks' doubles in block order, one rounding
        const int e = t - 64;
        s_ema[e] = (float)sum_block_order(A.epart + e, A.nblocks, kEmaValues);
    } else if (t == 128 && A.loss) {
        A.loss[0] = A.render_loss ? A.render_loss[0] : 0.0f;
        A.loss[1] = A.render_loss ? A.render_loss[1] : 0.0f;
        A.loss[2] = A.commit_sums ? A.commit_sums[0] : 0.0f;
        A.loss[3] = A.commit_sums ? A.commit_sums[1] : 0.0f;
    }
    if (!upd) return;  // (uniform)
    __syncthreads();
    // ResidualVQ8.ema_update, per stage: the moving averages of (stage, codeword) t
    float emb[3] = {0.0f, 0.0f, 0.0f};
    if (t < kStages * kCodewords) {
        const float cs = fmaf(A.one_m_decay, s_ema[4 * t], A.cluster[t] * A.decay);
        A.cluster[t] = cs;
        s_cluster[t] = cs;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            emb[k] = fmaf(A.one_m_decay, s_ema[4 * t + 1 + k], A.embed[3 * t + k] * A.decay);
            A.embed[3 * t + k] = emb[k];
        }
    }
    __syncthreads();
    if (t < kStages * kCodewords) {
        const int s0 = t & ~(kCodewords - 1);
        float total = s_cluster[s0];
        for (int j = 1; j < kCodewords; ++j) total = total + s_cluster[s0 + j];
        const float smoothed = ((s_cluster[t] + A.eps) / (total + A.eps_all)) * total;
#pragma unroll
        for (int k = 0; k < 3; ++k) A.cb[3 * t + k] = emb[k] / smoothed;
    }
}

// the step's own workspace: the quantizer's outputs, the gradient records, the partials
struct QuantTrainWs {
    float *xq, *Lq, *cq, *rec, *fwd_partials, *words, *partials;
    double *epart;
    unsigned char *codes_chol, *codes_rgb;
    size_t bytes;
};

static QuantTrainWs quant_train_ws(char *base, int num_points) {
    const size_t n = (size_t)(num_points > 0 ? num_points : 0);
    const size_t blocks = (size_t)quant_blocks(num_points);
    QuantTrainWs w;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char *p = base ? base + off : nullptr;
        off += ws_align(bytes);
        return p;
    };
    w.epart = (double *)take(sizeof(double) * kEmaValues * blocks);
    w.xq = (float *)take(sizeof(float) * 2 * n);
    w.Lq = (float *)take(sizeof(float) * 3 * n);
    w.cq = (float *)take(sizeof(float) * 3 * n);
    w.rec = (float *)take(sizeof(float) * 9 * n);
    w.fwd_partials = (float *)take(sizeof(float) * kQuantSums * blocks);
    w.partials = (float *)take(sizeof(float) * kQuantSums * blocks);
    w.words = (float *)take(sizeof(float) * 4);  // commitment sums [2], render losses [2]
    w.codes_chol = (unsigned char *)take(3 * n);
    w.codes_rgb = (unsigned char *)take(2 * n);
    w.bytes = off;
    return w;
}

// What gsvc_quant_train_step and gsvc_quant_adan_step share: the arguments of
// steps 3 and 4.
static int quant_train_check(const gsvc_quant_train_args *a, const char *what) {
    if (!a) return set_error(GSVC_ERR_ARG, "%s: null arguments", what);
    if (a->num_points < 1) return set_error(GSVC_ERR_ARG, "%s: num_points < 1", what);
    if (!a->xyz || !a->cholesky || !a->features)
        return set_error(GSVC_ERR_ARG, "%s: null parameter tensor", what);
    if (!a->scale || !a->beta) return set_error(GSVC_ERR_ARG, "%s: null scale / beta", what);
    if (!a->codebooks || !a->cluster_size || !a->embed_avg)
        return set_error(GSVC_ERR_ARG, "%s: null codebooks / cluster_size / embed_avg", what);
    if (!a->adan_hparams) return set_error(GSVC_ERR_ARG, "%s: missing Adan hyper-parameters", what);
    if (a->flags & ~(0x3f | GSVC_TRAIN_DETERMINISTIC))
        return set_error(GSVC_ERR_ARG, "%s: unknown flags 0x%x", what, a->flags);
    if (!a->grads_out) {
        if (!a->adan_state) return set_error(GSVC_ERR_ARG, "%s: missing Adan state", what);
        for (int k = 0; k < 20; ++k)
            if (!a->adan_state[k]) return set_error(GSVC_ERR_ARG, "%s: missing Adan state tensor", what);
        if (!(a->decay >= 0.0 && a->decay <= 1.0) || !(a->eps >= 0.0))
            return set_error(GSVC_ERR_ARG, "%s: decay in [0, 1] and eps >= 0 expected", what);
    }
    if (!(a->commitment_weight == a->commitment_weight))
        return set_error(GSVC_ERR_ARG, "%s: commitment_weight is NaN", what);
    if (!a->workspace || a->workspace_bytes < gsvc_quant_train_workspace_bytes(a->num_points))
        return set_error(GSVC_ERR_WORKSPACE, "%s: workspace of %zu bytes, need %zu", what,
                         a->workspace ? a->workspace_bytes : (size_t)0,
                         gsvc_quant_train_workspace_bytes(a->num_points));
    return GSVC_OK;
}

// steps 3 and 4
static int quant_adan_launch(const gsvc_quant_train_args *a, const QuantTrainWs &w, const float *rec,
                             const unsigned char *codes_rgb, const float *render_loss,
                             const float *commit_sums, const char *what) {
    hipStream_t s = (hipStream_t)a->stream;
    const int n = a->num_points, blocks = quant_blocks(n);
    const bool update = a->grads_out == nullptr;
    const double *h = a->adan_hparams;
    const AdanScalars S = adan_scalars(h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8],
                                       a->flags & 1, h[9]);
    QuantTrainSplatArgs P{};
    P.n = n;
    P.update = update ? 1 : 0;
    P.xyz = a->xyz;
    P.chol = a->cholesky;
    P.feat = a->features;
    P.scale = a->scale;
    P.beta = a->beta;
    P.cb = a->codebooks;
    P.codes_rgb = codes_rgb;
    P.rec = rec;
    P.vc = (float)(a->commitment_weight / (3.0 * (double)n));
    if (update)
        for (int q = 0; q < 3; ++q)
            for (int k = 0; k < 4; ++k) P.state[q][k] = a->adan_state[4 * q + k];
    for (int q = 0; q < 3; ++q) P.first[q] = (a->flags >> (1 + q)) & 1;
    P.S = S;
    P.grads_out = a->grads_out;
    P.partials = w.partials;
    P.epart = w.epart;
    hipLaunchKernelGGL(quant_train_splat_kernel, dim3(blocks), dim3(kQuantBlock), 0, s, P);
    int rc = check_launch(what);
    if (rc) return rc;
    QuantTrainFinishArgs F{};
    F.nblocks = blocks;
    F.update = update ? 1 : 0;
    F.partials = w.partials;
    F.epart = w.epart;
    F.scale = a->scale;
    F.beta = a->beta;
    if (update)
        for (int q = 0; q < 2; ++q)
            for (int k = 0; k < 4; ++k) F.state[q][k] = a->adan_state[4 * (3 + q) + k];
    for (int q = 0; q < 2; ++q) F.first[q] = (a->flags >> (4 + q)) & 1;
    F.S = S;
    F.cb = a->codebooks;
    F.cluster = a->cluster_size;
    F.embed = a->embed_avg;
    // torch takes the Python scalars decay, 1 - decay, eps, 8 * eps as fp32
    F.decay = (float)a->decay;
    F.one_m_decay = (float)(1.0 - a->decay);
    F.eps = (float)a->eps;
    F.eps_all = (float)((double)kCodewords * a->eps);
    F.render_loss = render_loss;
    F.commit_sums = commit_sums;
    F.loss = a->loss;
    F.grads_tail = update ? nullptr : a->grads_out + 8 * (size_t)n;
    hipLaunchKernelGGL(quant_train_finish_kernel, dim3(1), dim3(kQuantBlock), 0, s, F);
    return check_launch(what);
}

}  // namespace gsvc

using namespace gsvc;

extern "C" size_t gsvc_quant_train_workspace_bytes(int num_points) {
    return quant_train_ws(nullptr, num_points).bytes;
}

extern "C" int gsvc_quant_train_step(const gsvc_quant_train_args *a) {
    const char *what = "quant_train_step";
    int rc = quant_train_check(a, what);
    if (rc) return rc;
    if (!a->cholesky_bound) return set_error(GSVC_ERR_ARG, "%s: null cholesky_bound", what);
    const int np = (a->p_xyz != nullptr) + (a->p_cholesky != nullptr) + (a->p_features != nullptr);
    if (np != 0 && np != 3)
        return set_error(GSVC_ERR_ARG, "%s: p_xyz, p_cholesky, p_features go together", what);
    if (!a->background || !a->gt) return set_error(GSVC_ERR_ARG, "%s: null background / gt", what);
    if (a->img_height == 0 || a->img_width == 0) return set_error(GSVC_ERR_ARG, "%s: bad sizes", what);
    if (a->loss_kind != 0 && a->loss_kind != 1)
        return set_error(GSVC_ERR_ARG, "%s: loss_kind must be 0 (L2) or 1 (L1)", what);
    if (!a->loss) return set_error(GSVC_ERR_ARG, "%s: null loss", what);
    const size_t need = gsvc_train_step_workspace_bytes(a->num_points, a->img_height, a->img_width);
    if (!a->train_workspace || a->train_workspace_bytes < need)
        return set_error(GSVC_ERR_WORKSPACE, "%s: train workspace of %zu bytes, need %zu", what,
                         a->train_workspace ? a->train_workspace_bytes : (size_t)0, need);
    const bool det = (a->flags & GSVC_TRAIN_DETERMINISTIC) != 0;
    if (det && (!a->det_workspace || a->det_capacity < 0 ||
                a->det_workspace_bytes <
                    gsvc_train_step_det_workspace_bytes(a->num_points, a->det_capacity)))
        return set_error(GSVC_ERR_WORKSPACE, "%s: GSVC_TRAIN_DETERMINISTIC needs a det_workspace of "
                                             "gsvc_train_step_det_workspace_bytes", what);
    hipStream_t s = (hipStream_t)a->stream;
    if ((rc = refuse_capture(s, what))) return rc;

    const QuantTrainWs w = quant_train_ws((char *)a->workspace, a->num_points);
    float *commit_sums = w.words, *render_loss = w.words + 2;
    // 1. the quantizer forward with its commitment sums
    rc = launch_quant_forward_train(what, a->num_points, a->xyz, a->cholesky, a->features, a->scale,
                                    a->beta, a->codebooks, a->cholesky_bound, a->p_xyz, a->p_cholesky,
                                    a->p_features, w.xq, w.Lq, w.cq, w.codes_chol, w.codes_rgb,
                                    w.fwd_partials, commit_sums, s);
    if (rc) return rc;
    // 2. the render step, gradients only: records [N,9] with respect to xq, Lq, cq
    gsvc_train_step_args T{};
    T.num_points = a->num_points;
    T.xyz = w.xq;
    T.cholesky = w.Lq;  // (holds cholesky_bound already)
    T.features = w.cq;
    T.background = a->background;
    T.gt = a->gt;
    T.img_height = a->img_height;
    T.img_width = a->img_width;
    T.loss_kind = a->loss_kind;
    T.frame_index = a->frame_index;
    T.adan_hparams = a->adan_hparams;
    T.adan_flags = det ? GSVC_TRAIN_DETERMINISTIC : 0;
    T.loss = render_loss;
    T.render_out = a->render_out;
    T.grads_out = w.rec;
    T.workspace = a->train_workspace;
    T.workspace_bytes = a->train_workspace_bytes;
    T.stream = a->stream;
    if (det) {
        T.det_workspace = a->det_workspace;
        T.det_workspace_bytes = a->det_workspace_bytes;
        T.det_capacity = a->det_capacity;
    }
    rc = gsvc_train_step_sum_args(&T);
    if (rc) return rc;
    // 3, 4. the quantizer's backward, Adan, the codebooks' moving average, the loss words
    return quant_adan_launch(a, w, w.rec, w.codes_rgb, render_loss, commit_sums, what);
}

extern "C" int gsvc_quant_adan_step(const gsvc_quant_train_args *a, const float *grad_records,
                                    const unsigned char *codes_rgb, const float *commit_sums) {
    const char *what = "quant_adan_step";
    const int rc = quant_train_check(a, what);
    if (rc) return rc;
    if (!grad_records || !codes_rgb)
        return set_error(GSVC_ERR_ARG, "%s: null grad_records / codes_rgb", what);
    const QuantTrainWs w = quant_train_ws((char *)a->workspace, a->num_points);
    return quant_adan_launch(a, w, grad_records, codes_rgb, nullptr, commit_sums, what);
}
