"""Inputs, the float64 restatement of ``ResidualVQ8.ema_update`` and the raw
call of the fused quantized step's quantizer half, shared by
test_quant_train_cpu.py and test_quant_train_gpu.py.  The restatement imports
nothing from the code under test: it is numpy float64 on the fp32 inputs (the
codebooks' member counts, member sums, the moving averages, the smoothing and
the division), plus the fp32 statement of ``cluster_size`` alone, whose inputs
are integers and which is therefore held exactly."""
import ctypes
import math

import numpy as np

import quant_cases as Q

F32 = np.float32
U = 2.0 ** -24
DECAY, EPS = 0.8, 1e-5
SIZES = [1, 63, 64, 65, 257, 4099]  # the project's wave and block edges
BIG = 1024 * 256 + 65                # the grid's stride loop takes a second, partial pass
LR = 1e-2
BETAS = (0.98, 0.92, 0.99)
COMMIT_WEIGHT = 0.37                 # not 1: the weight reaches the gradients


def ema_ref64(x, codes, cb, cluster, embed, decay=DECAY, eps=EPS):
    """ema_update in float64 from fp32 inputs: dict of cluster_size [2,8],
    embed_avg [2,8,3], codebooks [2,8,3], and per stage the member counts
    (int64) and the sums of the members' absolute values (for error bounds)."""
    r = x.astype(np.float64)
    cb64 = cb.astype(np.float64)
    cs, em, out = cluster.astype(np.float64).copy(), embed.astype(np.float64).copy(), np.zeros((2, 8, 3))
    counts, abs_sums = np.zeros((2, 8), np.int64), np.zeros((2, 8, 3))
    for s in range(2):
        idx = codes[:, s].astype(np.int64)
        for j in range(8):
            m = r[idx == j]
            counts[s, j] = m.shape[0]
            abs_sums[s, j] = np.abs(m).sum(0)
            cs[s, j] = cs[s, j] * decay + (1 - decay) * m.shape[0]
            em[s, j] = em[s, j] * decay + (1 - decay) * m.sum(0)
        total = cs[s].sum()
        smoothed = (cs[s] + eps) / (total + 8 * eps) * total
        out[s] = em[s] / smoothed[:, None]
        r = r - cb64[s][idx]
    return dict(cluster_size=cs, embed_avg=em, codebooks=out, counts=counts, abs_sums=abs_sums)


def cluster_size_f32(cluster, counts, decay=DECAY):
    """cluster_size as fp32 computes it, two roundings: cs * d, then the fused
    (1 - d) * counts + that (torch's add_(counts, alpha=1 - d); the kernel's
    fmaf).  counts < 2^24 and 1 - d are fp32, so their product is exact in
    float64 and so is its sum with a term of like size: one rounding to fp32."""
    r1 = (cluster.astype(F32) * F32(decay)).astype(F32)
    return (r1.astype(np.float64) + float(F32(1 - decay)) * counts.astype(np.float64)).astype(F32)


def rel_err(got, ref64):
    """max |got - ref| over the tensor, in units of the tensor's largest |ref|."""
    return float(np.abs(got.astype(np.float64) - ref64).max() / max(np.abs(ref64).max(), 1e-300))


def ema_bounds(ref, n, cluster, embed, decay=DECAY, eps=EPS):
    """Bounds on |fp32 ema_update - float64| for embed_avg and codebooks, for
    ANY summation order of the member sums: a sum of k terms has error at most
    (k - 1) u / (1 - (k - 1) u) sum|t| (+ u |t| per stage-1 member, whose
    residual f - e0 is itself rounded); the moving average adds 2 roundings of
    its two terms; smoothed is within 32 u (8 cluster sizes of 2 roundings, 7
    additions, 4 more ops); the division adds one rounding."""
    k = np.maximum(ref["counts"] - 1, 0)[..., None].astype(np.float64)
    sum_err = (k * U / (1 - k * U) + U) * ref["abs_sums"]
    em = np.abs(embed.astype(np.float64)) * decay + (1 - decay) * ref["abs_sums"]
    embed_err = (1 - decay) * sum_err + 4 * U * em
    cs = ref["cluster_size"]
    total = cs.sum(1, keepdims=True)
    smoothed = ((cs + eps) / (total + 8 * eps) * total)[..., None]
    cb_err = (embed_err + np.abs(ref["embed_avg"]) * 33 * U) / smoothed * (1 + 64 * U)
    return embed_err, cb_err


def half_case(n, delta, t, seed=0):
    """Inputs of the quantizer half on its own: quant_cases' parameters and
    tables, its upstream gradients as the render step's records [N,9], a
    codebook state mid-training, and for t = 2 a non-zero Adan state."""
    case = Q.make_case(n, seed=seed, delta=delta)
    rng = np.random.default_rng(9000 + 31 * n + 7 * t + (3 if delta else 0))
    v_xq, v_Lq, v_cq, _ = Q.upstream(n)
    rec = np.concatenate([v_xq, v_Lq, v_cq, rng.standard_normal((n, 1)).astype(F32)], 1)
    cluster = rng.uniform(0.25, n / 8 + 1, (2, 8)).astype(F32)
    embed = (case["cb"] * cluster[..., None] + 0.05 * rng.standard_normal((2, 8, 3))).astype(F32)
    shapes = [(n, 2), (n, 3), (n, 3), (3,), (3,)]
    state = []
    for shp in shapes:
        if t == 1:
            state.append([np.zeros(shp, F32) for _ in range(4)])
        else:
            state.append([(0.1 * rng.standard_normal(shp)).astype(F32),
                          (0.01 * rng.random(shp)).astype(F32),
                          (0.1 * rng.standard_normal(shp)).astype(F32),
                          (0.3 * rng.standard_normal(shp)).astype(F32)])
    return dict(case=case, rec=np.ascontiguousarray(rec), cluster=cluster, embed=embed, state=state, t=t,
                n=n)


def hparams(t, lr=LR, weight_decay=0.0, eps=1e-8):
    b1, b2, b3 = BETAS
    return [b1, b2, b3, 1.0 - b1 ** t, 1.0 - b2 ** t, math.sqrt(1.0 - b3 ** t), lr, weight_decay,
            eps, 1.0]


def args_struct(n, **fields):
    """A gsvc_quant_train_args with the given fields (ints / pointers)."""
    from gsvc_amd.compress import _QuantStepArgs
    a = _QuantStepArgs()
    a.num_points = n
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def quant_adan_step(dev, params, tables, state, rec, codes_rgb, commit_sums, t, first,
                    commit_weight=COMMIT_WEIGHT, grads_out=None, loss=None):
    """gsvc_quant_adan_step on device tensors, in place: params = (xyz, chol,
    feat, scale, beta), tables = (codebooks, cluster_size, embed_avg), state =
    20 tensors.  Returns nothing; raises on a status."""
    import torch
    from gsvc_amd import _lib as L
    n = params[0].shape[0]
    ws = torch.empty((L.size("gsvc_quant_train_workspace_bytes", n),), dtype=torch.uint8, device=dev)
    st = (ctypes.c_void_p * 20)(*[s.data_ptr() for s in state])
    hp = (ctypes.c_double * 10)(*hparams(t))
    flags = 0
    if first:
        flags |= 0x3e
    a = args_struct(n, xyz=params[0].data_ptr(), cholesky=params[1].data_ptr(),
                    features=params[2].data_ptr(), scale=params[3].data_ptr(),
                    beta=params[4].data_ptr(), codebooks=tables[0].data_ptr(),
                    cluster_size=tables[1].data_ptr(), embed_avg=tables[2].data_ptr(),
                    adan_state=ctypes.addressof(st), adan_hparams=ctypes.addressof(hp), flags=flags,
                    decay=DECAY, eps=EPS, commitment_weight=commit_weight,
                    loss=None if loss is None else loss.data_ptr(),
                    grads_out=None if grads_out is None else grads_out.data_ptr(),
                    workspace=ws.data_ptr(), workspace_bytes=ws.numel(),
                    stream=L.stream(dev).value)
    L.call("gsvc_quant_adan_step", ctypes.byref(a), L.ptr(rec), L.ptr(codes_rgb), L.ptr(commit_sums))
    torch.cuda.synchronize()
