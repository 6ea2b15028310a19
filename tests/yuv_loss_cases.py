"""Cases, float64 references, error measures and bars of the weighted Y/U/V
training loss (``loss_type="YUV"``), shared by
test_yuv_loss_cpu.py (premises, no GPU) and test_yuv_loss_gpu.py (the fused
step of train.hip).

Built on tests/sum_cases.py without changing it: a case is one of its fused-step
builders under a new id (``S.register_fused``), so ``S.fused_case`` nudges it
until no decision of the float64 forward lies within its margin, and
``S.chain_np`` gives the forward and its fixed decisions (which pairs pass the
alpha cut, which values pass the clamp; the loss adds no decision of its own).
The loss and its gradient are stated twice, as that file states L2 / L1:

* ``yuv_reference``: the definition in numpy float64 -- block means, plane
  errors as means over blocks, L = sum w_k mse_k / sum w_k, the closed-form
  gradient 2 / (H W sum w) sum_k w_k M[k][c] mean_k -- carried to the
  parameters by ``S.raster_bwd_np`` and backward2d.cu's projection VJP
  (``param_grads``);
* ``yuv_autograd``: torch float64 autograd from the raw parameters through the
  forward with the decisions fixed (``S._raster_torch``), torch.clamp and the
  loss written with torch ops.

``yuv_chain`` is the kernel's folding (w'_k = 3 w_k / sum w, G[k][c] =
2 / (3 H W) w'_k M[k][c], the per-pixel sum of w'_k mean_k^2 over numel) over
the number format: in float64 it must equal the definition (the CPU file holds
it to 1e-12), in float32 with sequential sums it is the restatement the bars
come from.  Nothing here imports the code under test except ``spec_of``, which
hands the GPU tests the YuvLoss of a case.
"""
import numpy as np
import torch

import sum_cases as S

F32, F64 = np.float32, np.float64

# ---------------------------------------------------------------- the matrix, restated
# gsvc_yuv_format_table's nine output coefficients (yR yG yB, uR uG uB, vR vG
# vB) as 20-bit fixed point; the legacy triple (8-bit bt601 limited) keeps
# OpenCV's constants
_LEGACY = (269484, 528482, 102760, -155188, -305135, 460324, 460324, -385875, -74448)
_KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
CHROMA_CODE = {"420": 0, "422": 1, "444": 2}


def matrix_of(depth, matrix, full):
    """M [3, 3] float64, rows Y, U, V: the fixed-point table over 2^20."""
    if depth == 8 and matrix == "bt601" and not full:
        return np.array(_LEGACY, F64).reshape(3, 3) / 2.0 ** 20
    P = float((1 << depth) - 1)
    kr, kb = _KR_KB[matrix]
    kg = 1.0 - kr - kb
    yspan = P if full else float(219 << (depth - 8))
    cspan = P if full else float(224 << (depth - 8))
    fix = lambda x: float(np.floor(x * 1048576.0 + 0.5))  # noqa: E731
    half = fix(cspan / (2.0 * P))
    t = (fix(kr * yspan / P), fix(kg * yspan / P), fix(kb * yspan / P),
         fix(-kr / (2.0 * (1.0 - kb)) * cspan / P), fix(-kg / (2.0 * (1.0 - kb)) * cspan / P), half,
         half, fix(-kg / (2.0 * (1.0 - kr)) * cspan / P), fix(-kb / (2.0 * (1.0 - kr)) * cspan / P))
    return np.array(t, F64).reshape(3, 3) / 2.0 ** 20


# ---------------------------------------------------------------- cases
# id: (sum_cases builder, (depth, matrix, full range, chroma), weights).
# counts / span are 58x74 (4 x 5 tiles, 10 rows and 10 columns in the last
# ones): even, so they take 4:2:0 as they are.  The small frames: one block
# (2x2), one block row / column (2x38, 38x2: three tiles, the last of 6 pixels),
# a second tile row of two rows (18x16), partial tiles on both edges with the
# band edge at rows 7 | 8 inside a block row pair boundary (34x18, 38x46).
# 37x46 has an odd height (4:2:2), the sum_cases shapes 1x1, 17x15, 37x45 are
# odd both ways (4:4:4).  counts' colours reach 20: blocks with one, two or
# three clamped pixels; `empty` has no visible splat (M < 1).
LEGACY_FMT = (8, "bt601", False)
CASES = {
    "counts-420": ("counts", LEGACY_FMT + ("420",), (6.0, 1.0, 1.0)),
    "counts-rgbw-420": ("counts-rgbw", (8, "bt709", True, "420"), (1.0, 1.0, 1.0)),
    "span-420": ("span", (10, "bt709", False, "420"), (6.0, 1.0, 1.0)),
    "2x2-420": ("shape-2x2", LEGACY_FMT + ("420",), (6.0, 1.0, 1.0)),
    "2x38-420": ("shape-2x38", (8, "bt709", True, "420"), (1.0, 0.0, 0.0)),
    "38x2-420": ("shape-38x2", (10, "bt601", False, "420"), (6.0, 1.0, 1.0)),
    "18x16-420": ("shape-18x16", LEGACY_FMT + ("420",), (1.0, 1.0, 1.0)),
    "34x18-420": ("shape-34x18", (8, "bt709", True, "420"), (6.0, 1.0, 1.0)),
    "38x46-420": ("shape-38x46", (10, "bt709", True, "420"), (6.0, 1.0, 1.0)),
    "37x46-422": ("shape-37x46", (10, "bt601", False, "422"), (6.0, 1.0, 1.0)),
    "1x1-444": ("shape-1x1", LEGACY_FMT + ("444",), (6.0, 1.0, 1.0)),
    "17x15-444": ("shape-17x15", (8, "bt709", True, "444"), (1.0, 1.0, 1.0)),
    "37x45-444": ("shape-37x45", (10, "bt709", False, "444"), (1.0, 0.0, 0.0)),
    "empty-420": ("empty", LEGACY_FMT + ("420",), (6.0, 1.0, 1.0)),
}
IDS = list(CASES)
COUNT_IDS = ["counts-420", "counts-rgbw-420"]  # the per-tile measure is on


def _builder(cid):
    return S._build_fused(CASES[cid[4:]][0])


for _cid in IDS:
    if "yuv-" + _cid not in S._extra_builders:
        S.register_fused("yuv-" + _cid, _builder)


def case(cid):
    """(p, r, spec): the nudged parameters, S.chain_np's float64 result (its
    loss fields are L2's and not used) and the loss's spec as a dict: M [3,3]
    float64, w [3], chroma code, the format."""
    p, r = S.fused_case("yuv-" + cid)
    _, fmt, w = CASES[cid]
    return p, r, dict(M=matrix_of(*fmt[:3]), w=np.array(w, F64), chroma=CHROMA_CODE[fmt[3]], fmt=fmt)


def spec_of(cid):
    """The case's gsvc_amd.video.YuvLoss (for the code under test)."""
    from gsvc_amd.video import YuvFormat, YuvLoss
    _, fmt, w = CASES[cid]
    return YuvLoss(YuvFormat(*fmt), w)


# ---------------------------------------------------------------- the loss, twice
def _blocks(chroma):
    return (2 if chroma == 0 else 1), (1 if chroma == 2 else 2)


def yuv_definition(img, gt, spec):
    """The issue's definition in float64: (plane mse [3], L, dL/dimg [3, H, W])
    for img = the clamped render, with no clamp rule applied yet."""
    img, gt = np.asarray(img, F64), np.asarray(gt, F64)
    _, H, W = img.shape
    M, w = spec["M"], spec["w"]
    by, bx = _blocks(spec["chroma"])
    e = np.einsum("kc,chw->khw", M, img - gt)
    mean = [e[0]] + [e[k].reshape(H // by, by, W // bx, bx).mean(axis=(1, 3)) for k in (1, 2)]
    mse = np.array([(m * m).mean() for m in mean])
    L = float((w * mse).sum() / w.sum())
    up = [mean[0]] + [np.repeat(np.repeat(m, by, 0), bx, 1) for m in mean[1:]]
    g = np.zeros_like(img)
    for c in range(3):
        g[c] = 2.0 / (H * W * w.sum()) * sum(w[k] * M[k, c] * up[k] for k in range(3))
    return mse, L, g


def yuv_chain(img, gt, spec, dt=F64, seq=False):
    """The kernel's folding over the number format: (L, v_img [3, H, W]) from
    w'_k = 3 w_k / sum w, G[k][c] = 2 / (3 H W) w'_k M[k][c] (double, rounded
    once to dt), the block sums in the order (row's pair) + (other row's pair),
    and L = sum over pixels of sum_k w'_k mean_k^2, over numel."""
    f = dt
    img, gt = img.astype(dt), gt.astype(dt)
    _, H, W = img.shape
    numel = 3 * H * W
    M64, w = spec["M"], spec["w"]
    wp64 = 3.0 * w / w.sum()
    M, wp = M64.astype(dt), wp64.astype(dt)
    G = ((2.0 / numel) * wp64[:, None] * M64).astype(dt)
    by, bx = _blocks(spec["chroma"])
    d = img - gt
    e = [(M[k, 0] * d[0] + M[k, 1] * d[1]) + M[k, 2] * d[2] for k in range(3)]
    mean = [e[0]]
    for k in (1, 2):
        x = e[k].reshape(H // by, by, W // bx, bx)
        s = x[:, 0, :, 0]
        if bx == 2:
            s = s + x[:, 0, :, 1]
        if by == 2:
            s = s + (x[:, 1, :, 0] + x[:, 1, :, 1])
        s = s * f(1.0 / (by * bx))
        mean.append(np.repeat(np.repeat(s, by, 0), bx, 1).astype(dt))
    t = ((wp[0] * mean[0]) * mean[0] + (wp[1] * mean[1]) * mean[1]) + (wp[2] * mean[2]) * mean[2]
    L = float(S._acc(t.reshape(-1).astype(dt), 0, seq)) / numel
    v = np.stack([(G[0, c] * mean[0] + G[1, c] * mean[1]) + G[2, c] * mean[2] for c in range(3)]).astype(dt)
    return L, v


def param_grads(p, r, v_out, dt=F64, seq=False):
    """v_out [H, W, 3] (already zero where the clamp does not pass) carried to
    the parameters: S.raster_bwd_np, then backward2d.cu:8-51 (v_cov = -X G X,
    the Cholesky cross term doubled as there) and the activations' derivatives
    -- chain_np's own lines, for any v_out."""
    f = dt
    H, W = p["H"], p["W"]
    n = p["xyz"].shape[0]
    pr, L, means = r["proj"], r["L"], r["means"]
    feat, rgbw = p["feat"].astype(dt), p["rgbw"].astype(dt)
    G = S.raster_bwd_np(r["c"], r["fwd"], pr["conic"], r["colors"], np.ones(n, dt), v_out.astype(dt), dt, seq)
    X00, X01, X11 = pr["conic"][:, 0], pr["conic"][:, 1], pr["conic"][:, 2]
    G00, G01, G11 = G[:, 2], G[:, 3], G[:, 4]
    P00, P01 = -X00 * G00 - X01 * G01, -X01 * G00 - X11 * G01
    P10, P11 = -X00 * G01 - X01 * G11, -X01 * G01 - X11 * G11
    V00, V01 = P00 * X00 + P10 * X01, P01 * X00 + P11 * X01
    V10, V11 = P00 * X01 + P10 * X11, P01 * X01 + P11 * X11
    g11, g12, g22 = V00, V10 + V01, V11
    l11, l21, l22 = L[:, 0], L[:, 1], L[:, 2]
    two = f(2.0)
    grads = np.zeros((n, 9), dt)
    grads[:, 0] = (G[:, 0] * (f(0.5) * f(W))) * (f(1.0) - means[:, 0] * means[:, 0])
    grads[:, 1] = (G[:, 1] * (f(0.5) * f(H))) * (f(1.0) - means[:, 1] * means[:, 1])
    grads[:, 2] = two * l11 * g11 + two * g12 * l21
    grads[:, 3] = two * l11 * g12 + two * l21 * g22
    grads[:, 4] = two * l22 * g22
    grads[:, 5:8] = G[:, 5:8] * rgbw
    if p["rgbw_train"]:
        grads[:, 8] = (G[:, 5] * feat[:, 0] + G[:, 6] * feat[:, 1]) + G[:, 7] * feat[:, 2]
    grads[~pr["ok"]] = 0
    return grads


def _finish(p, r, v_img, dt, seq):
    n = p["xyz"].shape[0]
    if r["M"] < 1:
        return np.zeros((n, 9), dt)
    v_out = np.where(r["passes"], v_img.transpose(1, 2, 0), dt(0.0)).astype(dt)
    return param_grads(p, r, v_out, dt, seq)


_ref_cache = {}


def yuv_reference(cid):
    """The float64 reference of a case by the definition: dict(render, mse (the
    RGB one), plane [3], loss, grads [N, 9])."""
    if cid not in _ref_cache:
        p, r, spec = case(cid)
        gt = p["gt"].astype(F64).reshape(3, p["H"], p["W"])
        plane, L, g = yuv_definition(r["render"], gt, spec)
        _ref_cache[cid] = dict(render=r["render"], mse=r["losses"][0], plane=plane, loss=L,
                               grads=_finish(p, r, g, F64, False))
    return _ref_cache[cid]


def yuv_folded(cid, dt=F64, seq=False):
    """(render, (mse, L), grads) by the kernel's folding in the format dt."""
    p, _, spec = case(cid)
    r = S.chain_np(p, dt, seq)
    gt = p["gt"].astype(dt).reshape(3, p["H"], p["W"])
    L, v = yuv_chain(r["render"], gt, spec, dt, seq)
    return r["render"], (r["losses"][0], L), _finish(p, r, v, dt, seq)


def _yuv_loss_torch(img, gt, spec):
    M, w = torch.from_numpy(spec["M"]), torch.from_numpy(spec["w"])
    _, H, W = img.shape
    by, bx = _blocks(spec["chroma"])
    e = torch.einsum("kc,chw->khw", M, img - gt)
    mse = [(e[0] ** 2).mean()] + [(e[k].reshape(H // by, by, W // bx, bx).mean(dim=(1, 3)) ** 2).mean()
                                  for k in (1, 2)]
    return (w * torch.stack(mse)).sum() / w.sum()


def yuv_autograd(cid):
    """S.train_grads64_autograd with the loss replaced: (render, L, grads)."""
    p, ref, spec = case(cid)
    H, W = p["H"], p["W"]
    n = p["xyz"].shape[0]
    t = lambda a: torch.tensor(np.asarray(a, F64), dtype=torch.float64)  # noqa: E731
    gt = t(p["gt"]).reshape(3, H, W)
    if ref["M"] < 1:
        return ref["render"], float(_yuv_loss_torch(t(ref["render"]), gt, spec)), np.zeros((n, 9))
    xyz, chol, feat, rgbw = (t(p[k]).requires_grad_(True) for k in ("xyz", "chol", "feat", "rgbw"))
    ok = torch.from_numpy(ref["proj"]["ok"])
    means = torch.tanh(xyz)
    L = chol + t(p["bound"])[None, :]
    colors = feat * rgbw
    xy = torch.stack([0.5 * W * means[:, 0] + 0.5 * W, 0.5 * H * means[:, 1] + 0.5 * H], 1)
    cxx, cxy, cyy = L[:, 0] * L[:, 0], L[:, 0] * L[:, 1], L[:, 1] * L[:, 1] + L[:, 2] * L[:, 2]
    cxy.retain_grad()
    det = torch.where(ok, cxx * cyy - cxy * cxy, torch.ones_like(cxx))
    con = torch.stack([cyy / det, -cxy / det, cxx / det], 1)
    out = S._raster_torch(ref["c"], ref["fwd"], xy, con, colors, torch.ones(n, dtype=torch.float64))
    img = torch.clamp(out, 0, 1).permute(2, 0, 1)
    loss = _yuv_loss_torch(img, gt, spec)
    loss.backward()
    g12 = cxy.grad
    gl = chol.grad.clone()
    gl[:, 0] += g12 * L[:, 1].detach()
    gl[:, 1] += g12 * L[:, 0].detach()
    grads = torch.cat([xyz.grad, gl, feat.grad, rgbw.grad if p["rgbw_train"] else torch.zeros(n, 1,
                      dtype=torch.float64)], 1)
    grads[~ok] = 0
    return img.detach().numpy(), loss.item(), grads.numpy()


# ---------------------------------------------------------------- errors and bars
def yuv_errors(cid, render, losses, grads):
    """A step's result against yuv_reference: the render (absolute), word 0
    against the RGB mse (loss_abs / loss_rel), word 1 against L (yuv_loss_abs /
    yuv_loss_rel), and per parameter gradient S.grad_errors' (whole, edge,
    worst tile, that tile)."""
    p, r, _ = case(cid)
    ref = yuv_reference(cid)
    losses = np.asarray(losses, F64)
    d0, d1 = abs(losses[0] - ref["mse"]), abs(losses[1] - ref["loss"])
    e = dict(render=float(np.abs(np.asarray(render, F64).reshape(ref["render"].shape) - ref["render"]).max()),
             loss_abs=float(d0), loss_rel=float(d0 / ref["mse"]),
             yuv_loss_abs=float(d1), yuv_loss_rel=float(d1 / ref["loss"]))
    grads = np.asarray(grads, F64)
    for name, sl in S.PARAM_GRADS:
        e[name] = S.grad_errors(r["c"], grads[:, sl], ref["grads"][:, sl], per_tile=cid in COUNT_IDS)
    return e


KEYS = ("render", "loss_abs", "loss_rel", "yuv_loss_abs", "yuv_loss_rel") + tuple(n for n, _ in S.PARAM_GRADS)

# Bars, by sum_cases.py:55-85's rule: 4 x the worst error against float64 of the
# float32 restatement with sequential float32 sums (yuv_folded(cid, F32, True))
# over the cases above, measured on the CPU (tests/test_yuv_loss_cpu.py
# re-measures and holds the restatement to half its bars) before any GPU run.  The gradient's scale
# is not L2's (|G| <= 2 / numel x 3 w_k / sum w x |M|), so none of S.BARS' numbers
# is reused.  Gradients: the worst of the whole tensor, the edge subset and (on
# the counts cases) each tile's own splats.
#                  float32-seq   case of the worst      kernels' worst (MI355X)   case
#   render         6.63e-6       span-420               7.74e-6    counts-rgbw-420
#   loss_abs       7.12e-7       counts-420             3.07e-8    2x2-420
#   loss_rel       2.56e-6       counts-420             6.98e-8    2x2-420
#   yuv_loss_abs   2.38e-7       38x46-420              1.72e-8    1x1-444
#   yuv_loss_rel   2.12e-6       counts-rgbw-420        1.83e-7    counts-rgbw-420 (op path)
#   d_xyz          3.25e-5       counts-rgbw-420        4.52e-5    counts-rgbw-420, tile measure
#   d_cholesky     7.01e-5       counts-420             7.02e-5    counts-420 (op path)
#   d_features     3.12e-5       counts-rgbw-420        3.14e-5    counts-rgbw-420 (op path)
#   d_rgb_W        1.67e-4       counts-rgbw-420        1.68e-4    counts-rgbw-420 (op path)
# (as in sum_cases, the gradient figures are the one-entry tiles' of `counts`
# under the per-tile measure: colours up to 20 and centres near x = 70.)
WORST = dict(render=6.63e-06, loss_abs=7.12e-07, loss_rel=2.56e-06, yuv_loss_abs=2.38e-07,
             yuv_loss_rel=2.12e-06, d_xyz=3.25e-05, d_cholesky=7.01e-05, d_features=3.12e-05,
             d_rgb_W=1.67e-04)
BARS = {k: 4.0 * v for k, v in WORST.items()}


def measure_float32():
    """{key: (worst error, case)} of the float32-sequential restatement."""
    worst = {k: (0.0, "") for k in KEYS}
    for cid in IDS:
        e = yuv_errors(cid, *yuv_folded(cid, F32, True))
        for k in KEYS:
            v = S.worst_of(e, k)
            if v > worst[k][0]:
                worst[k] = (v, cid)
    return worst
