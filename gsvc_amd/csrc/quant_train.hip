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
// gsvc_quant_train_run enqueues K such steps in one call (the same two
// functions: quant_step_check, quant_step_enqueue) and, after each, the
// keep-best kernel below: the best state of the fine-tune stays on the device.
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
#include <stdio.h>

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
    unsigned *ticket;  // gsvc_quant_train_run's keep-best kernel: its arrival count
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
    w.ticket = (unsigned *)take(sizeof(unsigned));  // (last: the offsets above are the single step's)
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

// gsvc_quant_train_run's keep-best kernel: the reference's "best state"
// (train_video_Compress.py:89-102) without the host.  When this iteration's mse
// is below *best_mse (strictly; false for a NaN) the eight tensors, as the
// iteration left them, go to the snapshot, a grid-stride copy in 16-byte
// chunks where both ends allow it and in floats otherwise (2 N and 3 N are no
// multiples of 4 in general).  Every workgroup reads the pair once, through
// its lane 0, BEFORE it arrives at the ticket; the workgroup that arrives last
// -- after every read -- writes *best_mse and *best_iter, and the wrapping
// increment leaves the ticket at zero for the next launch.  A launch that does
// not take (the same decision in every workgroup: nothing has written the
// pair) returns at once and leaves the ticket alone.
constexpr int kKeepBlock = 256;
constexpr int kKeepMaxBlocks = 256;  // a CU each
constexpr int kKeepTensors = 8;
static_assert(3 + 3 + 7 * kStages * kCodewords <= kKeepBlock, "a lane per small-tensor float");

struct QuantKeepArgs {
    long long len[kKeepTensors];  // 2 N, 3 N, 3 N, 3, 3, 48, 16, 48
    const float *src[kKeepTensors];
    float *dst[kKeepTensors];
    const float *mse;  // the step's mean squared error (the word the finish kernel logs)
    float *best_mse;
    int *best_iter;
    unsigned *ticket;
    int iter;
};

__global__ __launch_bounds__(kKeepBlock) void quant_keep_best_kernel(QuantKeepArgs A) {
    __shared__ float s_pair[2];
    const int t = threadIdx.x;
    if (t == 0) {
        s_pair[0] = *A.mse;
        s_pair[1] = *A.best_mse;
    }
    __syncthreads();
    const float mse = s_pair[0];
    // uniform over the grid: every workgroup reads the pair before any write to it (below).
    // Without a take nothing is written and nobody needs to arrive.
    if (!(mse < s_pair[1])) return;
    const long long stride = (long long)gridDim.x * kKeepBlock;
    const long long t0 = (long long)blockIdx.x * kKeepBlock + t;
    // the three per-splat tensors: a pass loads a 16-byte chunk of each, then stores them
    // (one round trip for the three); a tensor whose ends are not 16-byte aligned has no chunks
    long long n4[3], most = 0;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const bool v4 = (((uintptr_t)A.dst[q] | (uintptr_t)A.src[q]) & 15u) == 0;
        n4[q] = v4 ? A.len[q] >> 2 : 0;
        most = n4[q] > most ? n4[q] : most;
    }
    for (long long i = t0; i < most; i += stride) {
        // (named registers: an array under these conditions is lowered to LDS, a wait per load)
        float4 c0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), c1 = c0, c2 = c0;
        if (i < n4[0]) c0 = reinterpret_cast<const float4 *>(A.src[0])[i];
        if (i < n4[1]) c1 = reinterpret_cast<const float4 *>(A.src[1])[i];
        if (i < n4[2]) c2 = reinterpret_cast<const float4 *>(A.src[2])[i];
        if (i < n4[0]) reinterpret_cast<float4 *>(A.dst[0])[i] = c0;
        if (i < n4[1]) reinterpret_cast<float4 *>(A.dst[1])[i] = c1;
        if (i < n4[2]) reinterpret_cast<float4 *>(A.dst[2])[i] = c2;
    }
    // what the chunks leave (2 N and 3 N are no multiples of 4 in general), float by float
#pragma unroll
    for (int q = 0; q < 3; ++q)
        for (long long i = 4 * n4[q] + t0; i < A.len[q]; i += stride) A.dst[q][i] = A.src[q][i];
    // the five small tensors, 118 floats: a lane of the last workgroup each
    if (blockIdx.x == gridDim.x - 1) {
        int k = t;
#pragma unroll
        for (int q = 3; q < kKeepTensors; ++q) {
            if (k >= 0 && k < (int)A.len[q]) A.dst[q][k] = A.src[q][k];
            k -= (int)A.len[q];
        }
    }
    if (t == 0) {
        // lane 0's reads of the pair are done (the branch above took them); the fence keeps
        // them ahead of the arrival, and the last arrival's writes behind every arrival
        __threadfence();
        const unsigned last = gridDim.x - 1;
        if (atomicInc(A.ticket, last) == last) {
            __threadfence();
            *A.best_mse = mse;
            *A.best_iter = A.iter;
        }
    }
}

static int blocks_of_keep(int n) {
    const long long chunks = (8LL * n + 3) / 4;
    const long long b = (chunks + kKeepBlock - 1) / kKeepBlock;
    return (int)(b < 1 ? 1 : b > kKeepMaxBlocks ? kKeepMaxBlocks : b);
}

}  // namespace gsvc

using namespace gsvc;

extern "C" size_t gsvc_quant_train_workspace_bytes(int num_points) {
    return quant_train_ws(nullptr, num_points).bytes;
}

// gsvc_quant_train_step's checks, all but the stream's
static int quant_step_check(const gsvc_quant_train_args *a, const char *what) {
    int rc = quant_train_check(a, what);
    if (rc) return rc;
    if (!a->cholesky_bound) return set_error(GSVC_ERR_ARG, "%s: null cholesky_bound", what);
    const int np = (a->p_xyz != nullptr) + (a->p_cholesky != nullptr) + (a->p_features != nullptr);
    if (np != 0 && np != 3)
        return set_error(GSVC_ERR_ARG, "%s: p_xyz, p_cholesky, p_features go together", what);
    if (!a->background || !a->gt) return set_error(GSVC_ERR_ARG, "%s: null background / gt", what);
    if (a->img_height == 0 || a->img_width == 0) return set_error(GSVC_ERR_ARG, "%s: bad sizes", what);
    if ((rc = loss_kind_check(what, a->loss_kind, a->loss_yuv, a->loss_chroma, a->img_height, a->img_width)))
        return rc;
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
    return GSVC_OK;
}

// gsvc_quant_train_step's launches, on checked arguments
static int quant_step_enqueue(const gsvc_quant_train_args *a, const char *what) {
    hipStream_t s = (hipStream_t)a->stream;
    const bool det = (a->flags & GSVC_TRAIN_DETERMINISTIC) != 0;
    int rc;
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
    T.loss_yuv = a->loss_yuv;
    T.loss_chroma = a->loss_chroma;
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

extern "C" int gsvc_quant_train_step(const gsvc_quant_train_args *a) {
    const char *what = "quant_train_step";
    int rc = quant_step_check(a, what);
    if (rc) return rc;
    if ((rc = refuse_capture((hipStream_t)a->stream, what))) return rc;
    return quant_step_enqueue(a, what);
}

// a failed launch of iteration i: the status, with the iteration ahead of the message
static int run_error(int rc, int i) {
    char msg[384];
    snprintf(msg, sizeof msg, "%s", gsvc_last_error());
    return set_error(rc, "quant_train_run: iteration %d: %s", i, msg);
}

extern "C" int gsvc_quant_train_run(const gsvc_quant_train_run_args *r) {
    const char *what = "quant_train_run";
    if (!r) return set_error(GSVC_ERR_ARG, "%s: null run arguments", what);
    if (!r->step) return set_error(GSVC_ERR_ARG, "%s: null step arguments", what);
    if (r->iterations < 1) return set_error(GSVC_ERR_ARG, "%s: iterations < 1", what);
    if (!r->adan_hparams) return set_error(GSVC_ERR_ARG, "%s: null adan_hparams [iterations][10]", what);
    if (!r->flags) return set_error(GSVC_ERR_ARG, "%s: null flags [iterations]", what);
    if (!r->loss_log) return set_error(GSVC_ERR_ARG, "%s: null loss_log [iterations][4]", what);
    float *const snap[kKeepTensors] = {r->best_xyz,   r->best_cholesky,  r->best_features,
                                       r->best_scale, r->best_beta,      r->best_codebooks,
                                       r->best_cluster_size, r->best_embed_avg};
    int set = (r->best_mse != nullptr) + (r->best_iter != nullptr);
    for (int q = 0; q < kKeepTensors; ++q) set += snap[q] != nullptr;
    if (set != 0 && set != kKeepTensors + 2)
        return set_error(GSVC_ERR_ARG, "%s: best_mse, best_iter and the eight snapshot buffers go "
                                       "together", what);
    const bool keep = set != 0;
    if (r->step->grads_out)
        return set_error(GSVC_ERR_ARG, "%s: grads_out is set; a run has no test-hook mode", what);
    const int K = r->iterations;
    for (int i = 1; i < K; ++i)
        if ((r->flags[i] ^ r->flags[0]) & GSVC_TRAIN_DETERMINISTIC)
            return set_error(GSVC_ERR_ARG, "%s: GSVC_TRAIN_DETERMINISTIC differs between iterations "
                                           "0 and %d", what, i);
    // the single step's checks, for every iteration's flags (the other fields do not change)
    gsvc_quant_train_args a = *r->step;
    for (int i = 0; i < K; ++i) {
        a.adan_hparams = r->adan_hparams + 10 * (size_t)i;
        a.flags = r->flags[i];
        a.loss = r->loss_log + 4 * (size_t)i;
        const int rc = quant_step_check(&a, what);
        if (rc) return rc;
    }
    hipStream_t s = (hipStream_t)a.stream;
    int rc = refuse_capture(s, what);
    if (rc) return rc;

    const QuantTrainWs w = quant_train_ws((char *)a.workspace, a.num_points);
    QuantKeepArgs B{};
    int keep_blocks = 0;
    if (keep) {
        const long long n = a.num_points;
        const long long len[kKeepTensors] = {2 * n, 3 * n, 3 * n, 3, 3, kStages * kCodewords * 3,
                                             kStages * kCodewords, kStages * kCodewords * 3};
        const float *const src[kKeepTensors] = {a.xyz,  a.cholesky,  a.features,     a.scale,
                                                a.beta, a.codebooks, a.cluster_size, a.embed_avg};
        for (int q = 0; q < kKeepTensors; ++q) {
            B.len[q] = len[q];
            B.src[q] = src[q];
            B.dst[q] = snap[q];
        }
        B.mse = w.words + 2;  // the render step's {mse, mae}: loss_log[4 i] is a copy of this word
        B.best_mse = r->best_mse;
        B.best_iter = r->best_iter;
        B.ticket = w.ticket;
        keep_blocks = blocks_of_keep(a.num_points);
        if ((rc = dev_zero(w.ticket, sizeof(unsigned), s))) return run_error(rc, 0);
    }
    for (int i = 0; i < K; ++i) {
        a.adan_hparams = r->adan_hparams + 10 * (size_t)i;
        a.flags = r->flags[i];
        a.loss = r->loss_log + 4 * (size_t)i;
        a.frame_index = r->step->frame_index + i;
        if ((rc = quant_step_enqueue(&a, what))) return run_error(rc, i);
        if (keep) {
            B.iter = r->iter_base + i;
            hipLaunchKernelGGL(quant_keep_best_kernel, dim3(keep_blocks), dim3(kKeepBlock), 0, s, B);
            if ((rc = check_launch(what))) return run_error(rc, i);
        }
    }
    return GSVC_OK;
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
