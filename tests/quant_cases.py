"""Inputs and the in-test restatement shared by test_quantize_cpu.py and
test_quantize_gpu.py.  The reference imports nothing from the code under test
(only model_from_case, which builds its subject, does): it is numpy float32,
one rounding per op in the order DESIGN.md §13 states, and float64 sums."""
import numpy as np

F32 = np.float32
QMAX = 63
MARGIN = 1e-4  # nearest vs second-nearest squared distance, every non-tie colour

# power-of-two scales and dyadic betas: beta + raw * scale and its inverse are
# exact in fp32, so the constructed raw codes are hit exactly
SCALE = np.array([2.0 ** -4, 2.0 ** -5, 2.0 ** -3], F32)
BETA = np.array([-0.5, -0.25, 0.125], F32)
BOUND = np.array([0.5, 0.0, 0.5], F32)

# raw codes: below beta, above beta + 63 scale, on both clamp ends, k + 0.5 for
# even and odd k (round half to even), and halves next to the ends
HARD_RAW = np.array([-1.0, -0.25, 70.0, 63.25, 0.0, 63.0, 2.5, 3.5, 0.5, 1.5, 62.5, 61.5, 63.5, -0.5,
                     31.5, 32.5], F32)
# positions: ties between two halves (to even mantissa, both directions), a
# round-up into the next binade, the half subnormal range (spacing 2^-24) with
# its ties and its underflow to zero
HARD_XYZ = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2 - 2.0 ** -12, -(2 - 2.0 ** -12),
                     3e-6, -3e-6, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 2.0 ** -25, 1e-8,
                     2.0 ** -14 - 2.0 ** -26, 6.1e-5, 0.3330078125 + 2.0 ** -13, -1 - 2.0 ** -11], F32)


def codebooks():
    cb = np.zeros((2, 8, 3), F32)
    cb[0] = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0.5, 0.5, 1], [1, 0.25, 1],
             [0.25, 1, 0.75]]
    cb[1] = [[0, 0, 0], [0.2, 0, 0.05], [-0.2, 0.05, 0], [0, 0.2, -0.05], [0.05, -0.2, 0],
             [0, 0.05, 0.2], [-0.05, 0, -0.2], [0.15, 0.15, 0.15]]
    return cb


def _dist(r, cb):
    a = r[:, None, :] - cb[None, :, :]
    sq = a * a
    return (sq[..., 0] + sq[..., 1]) + sq[..., 2]


def _margins(f, cb):
    """float64 gap between nearest and second-nearest squared distance, per stage."""
    f = f.astype(np.float64)
    cb = cb.astype(np.float64)
    d0 = np.sort(_dist(f, cb[0]), axis=1)
    e0 = cb[0][np.argmin(_dist(f, cb[0]), axis=1)]
    d1 = np.sort(_dist(f - e0, cb[1]), axis=1)
    return d0[:, 1] - d0[:, 0], d1[:, 1] - d1[:, 0]


def make_case(n, seed=0, delta=False):
    rng = np.random.default_rng(seed + 1000 * n + (500 if delta else 0))
    cb = codebooks()
    xyz = (rng.standard_normal((n, 2)) * 1.2).astype(F32)
    raw = rng.uniform(-3, 66, (n, 3)).astype(F32)
    for i in range(min(n, len(HARD_RAW))):
        raw[i, :] = HARD_RAW[i]
    if n > 2 * len(HARD_RAW):  # and once more spread over the channels
        for i in range(len(HARD_RAW)):
            raw[len(HARD_RAW) + i, i % 3] = HARD_RAW[(i + 5) % len(HARD_RAW)]
    chol = (BETA[None] + raw * SCALE[None]).astype(F32)
    for i in range(min(n, len(HARD_XYZ))):
        xyz[n - 1 - i, i % 2] = HARD_XYZ[i]
    if n == 1:
        xyz[0] = [HARD_XYZ[0], HARD_XYZ[6]]
    # colours: rejection-sample away from every decision boundary of both stages
    feat = np.zeros((0, 3), F32)
    while feat.shape[0] < n:
        cand = rng.uniform(-0.2, 1.2, (4 * n + 64, 3)).astype(F32)
        m0, m1 = _margins(cand, cb)
        feat = np.concatenate([feat, cand[(m0 > 4 * MARGIN) & (m1 > 4 * MARGIN)]])
    feat = feat[:n].copy()
    tie = np.zeros(n, bool)
    feat[n // 2] = [0.5, 0, 0]  # equidistant from codewords 0 and 1 under any formula
    tie[n // 2] = True
    case = dict(n=n, xyz=xyz, chol=chol, feat=feat, scale=SCALE.copy(), beta=BETA.copy(), cb=cb,
                bound=BOUND.copy(), tie=tie, prev=None)
    if delta:
        case["prev"] = ((rng.standard_normal((n, 2)) * 0.7).astype(F32),
                        rng.uniform(0, 2, (n, 3)).astype(F32), rng.uniform(0, 1, (n, 3)).astype(F32))
    return case


def check_margins(case):
    """Every colour but the constructed tie keeps MARGIN at stage 0, and every
    colour at stage 1: rounding in the distance cannot change an index."""
    m0, m1 = _margins(case["feat"], case["cb"])
    assert (m0[~case["tie"]] > MARGIN).all(), m0[~case["tie"]].min()
    assert (m1 > MARGIN).all(), m1.min()
    assert (m0[case["tie"]] == 0).all()


def ref_forward(case):
    xyz, chol, feat = case["xyz"], case["chol"], case["feat"]
    scale, beta, cb, bound = case["scale"], case["beta"], case["cb"], case["bound"]
    xq = xyz.astype(np.float16).astype(F32)
    raw = (chol - beta[None]) / scale[None]
    q = np.rint(np.clip(raw, 0, QMAX)).astype(F32)
    Lpre = q * scale[None] + beta[None]
    Lq = Lpre + bound[None]
    d0 = _dist(feat, cb[0])
    i0 = np.argmin(d0, axis=1)  # first occurrence: the lowest index of equal distances
    e0 = cb[0][i0]
    r1 = feat - e0
    d1 = _dist(r1, cb[1])
    i1 = np.argmin(d1, axis=1)
    e1 = cb[1][i1]
    cq = e0 + e1
    if case["prev"] is not None:
        p = case["prev"]
        xq, Lq, Lpre, cq = xq + p[0], Lq + p[1], Lpre + p[1], cq + p[2]
    assert all(a.dtype == F32 for a in (xq, Lq, cq, raw, d0, d1))
    n = xyz.shape[0]
    return dict(xq=xq, Lq=Lq, Lpre=Lpre, cq=cq, codes_chol=q.astype(np.uint8),
                codes_rgb=np.stack([i0, i1], 1).astype(np.uint8), raw=raw, q=q, r1=r1, e1=e1,
                commit_terms=np.stack([d0[np.arange(n), i0], d1[np.arange(n), i1]], 1))


def ref_planes(xyz, codes_chol, codes_rgb):
    """The stream's two planes restated: N x (half x, half y), then N x 3 bytes
    of c0 | c1 << 6 | c2 << 12 | i0 << 18 | i1 << 21, little-endian."""
    cc, cr = codes_chol.astype(np.uint32), codes_rgb.astype(np.uint32)
    w = cc[:, 0] | cc[:, 1] << 6 | cc[:, 2] << 12 | cr[:, 0] << 18 | cr[:, 1] << 21
    b = np.stack([w & 255, (w >> 8) & 255, (w >> 16) & 255], 1).astype(np.uint8)
    return xyz.astype("<f2").tobytes() + b.tobytes()


def ref_backward(case, ref, v_xq, v_Lq, v_cq, v_commit):
    raw, q = ref["raw"], ref["q"]
    mask = ((raw >= 0) & (raw <= QMAX)).astype(F32)
    v_chol = v_Lq * mask
    t_scale = v_Lq * (q - mask * raw)
    t_beta = v_Lq * (F32(1) - mask)
    st = F32(2) * v_cq
    full = st + (v_commit[0] * (F32(2) * ref["r1"]) + v_commit[1] * (F32(2) * (ref["r1"] - ref["e1"])))
    assert all(a.dtype == F32 for a in (v_chol, t_scale, t_beta, st, full))
    return dict(v_xyz=v_xq, v_chol=v_chol, v_feat_st=st, v_feat=full, t_scale=t_scale, t_beta=t_beta)


def upstream(n, seed=7):
    rng = np.random.default_rng(seed + n)
    return (rng.standard_normal((n, 2)).astype(F32), rng.standard_normal((n, 3)).astype(F32),
            rng.standard_normal((n, 3)).astype(F32), np.array([0.37, -1.25], F32) / F32(3 * n))


def longest_path(n):
    """Additions on the longest path of the kernels' reduction as built
    (csrc/quant.hip): per lane ceil(n / (blocks * 256)) values in sequence
    (starting from 0), 6 xor-shuffle folds, 3 adds over the 4 wave sums, then
    blocks - 1 adds over the block partials."""
    blocks = max(1, min(-(-n // 256), 1024))
    per_lane = -(-n // (blocks * 256))
    return per_lane + 6 + 3 + (blocks - 1)


def sum_bound(terms):
    """|fp32 fixed-order sum - float64 sum| of these fp32 terms: (N - 1) u sum|t|
    holds for any order; the reduction's longest path gives a tighter count for
    large N.  u = 2^-24; the factor 1 / (1 - k u) of the exact bound is kept."""
    n = terms.shape[0]
    k = min(n - 1, longest_path(n))
    u = 2.0 ** -24
    return k * u / (1 - k * u) * np.abs(terms.astype(np.float64)).sum(0)


def model_from_case(case, H=40, W=72, device="cpu"):
    """The case's tensors in a frame model of the package under test (eval mode)."""
    import torch
    from gsvc_amd import compress as C
    T = torch.from_numpy
    n = case["n"]
    cls = C.GaussianVideoFrameQ if case["prev"] is None else C.GaussianVideoDelta
    m = cls(num_points=n, H=H, W=W, BLOCK_H=16, BLOCK_W=16, device=device, lr=1e-3, quantize=True,
            opt_type="adan")
    with torch.no_grad():
        m._xyz.copy_(T(case["xyz"]))
        m._cholesky.copy_(T(case["chol"]))
        m._features_dc.copy_(T(case["feat"]))
        m.cholesky_quantizer.scale.copy_(T(case["scale"]))
        m.cholesky_quantizer.beta.copy_(T(case["beta"]))
        m.features_dc_quantizer.codebooks.copy_(T(case["cb"]))
        m.features_dc_quantizer.initted.fill_(True)
        m.features_dc_quantizer._initted_host = None  # re-read the buffer
        if case["prev"] is not None:
            m.p_xyz.copy_(T(case["prev"][0]))
            m.p_cholesky.copy_(T(case["prev"][1]))
            m.p_features_dc.copy_(T(case["prev"][2]))
    return m.to(device).eval()
