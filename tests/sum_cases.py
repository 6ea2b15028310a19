"""Cases, float64 references, error measures and bars shared by
test_sum_cases_cpu.py (premises, no GPU), test_sum_edges.py (the HIP kernels
of gsvc_amd/csrc/raster_sum.hip and the fused training step of train.hip) and
tests/analysis/sum_bars.py (where the bars come from).

The references are plain numpy / torch float64 written from the reference's
forward.cu:512-627, backward.cu:696-862, foward2d.cu, backward2d.cu and
GaussianSplats_Represent.py:57-70,191-195; they import nothing from the code
under test and do not call the C oracle (which only projects and bins the
seeded frames the op-level cases start from, as alpha_cases._frame does).

Every gradient is stated twice: `chain_np` (the formulas of backward.cu and
backward2d.cu written out, numpy) and torch autograd of the forward with every
decision -- which (entry, pixel) pairs pass the alpha cut, which pixels pass
the clamp, sgn(d) -- fixed to the float64 forward's.  Three quirks of the
reference are kept and stated, not hidden:

* backward.cu:832-834 gives v_conic.y = 1/2 v_sigma dx dy, HALF the derivative
  of sigma = 1/2 (a dx^2 + c dy^2) + b dx dy by b; autograd's cross term is
  halved to match.  (With G01 = G10 = v_conic.y, backward2d.cu's -X G X is then
  the true gradient by the symmetric covariance.)
* backward2d.cu:39-40 doubles the cross term of the Cholesky VJP: v_l11 = 2 l11
  g11 + 2 g12 l21 and v_l21 = 2 l11 g12 + 2 l21 g22, where the derivative of
  cxy = l11 l21 contributes g12 l21 and g12 l11.  Autograd reads g12 off the
  retained covariance and adds the second g12 l21 / g12 l11.
* alpha = min(1, o e^-sigma) (forward.cu:599), and the backward lets the
  gradient through that clamp (v_sigma = -o e^-sigma v_alpha whatever alpha):
  autograd takes the clamp straight through.  Only the `opacities` case (o =
  1.5) reaches it.

`chain_np` is written once over the number format: float64 is the reference;
float32 with every sum taken sequentially in pixel order (np.cumsum) is the
second float32 restatement tests/analysis/sum_bars.py measures next to the C
oracle -- the least favourable honest summation.
"""
import math

import numpy as np
import torch

import alpha_cases as A
from alpha_cases import _frame, _nearest, _set_lists, _tiles, rel_error  # noqa: F401 (shared builders)

F32, F64, I32 = np.float32, np.float64, np.int32
TILE = 16
TILE_PIX = 256       # only a tile's first 256 list entries blend (forward.cu:569-571,613)
ALPHA_MIN = 1.0 / 255.0
MARGIN = 1e-4        # relative distance of the cut, a radius or a tile box from its threshold
SIGMA_MARGIN = 1e-6  # |sigma| below this: the sigma < 0 test is borderline
CLAMP_MARGIN = 1e-5  # absolute distance of a clamped value from 0 / 1, and of |d| from 0 (L1)
EDGE_PX = 4.0        # splats centred within this of the right / bottom edge: the edge subset
MASK_CAP = 3e-4      # the borderline mask covers at most 0.03 % of an op-level case's pixels
BOUND = np.array([0.5, 0.0, 0.5], F32)

# ---------------------------------------------------------------- bars
# 4 x the worse of two float32 restatements' worst errors against float64 over
# every case (tests/analysis/sum_bars.py prints them): the C oracle (sums in
# double) and chain_np in float32 with sequential float32 sums.  Image and
# losses absolute (losses relative), each gradient relative to the reference's
# largest element -- the worst of the whole tensor, the edge subset and, on the
# counts cases, each tile's own splats against that tile's largest element.
# The factor covers the kernels' summation trees (DPP segments, float atomics),
# fma contraction and v_exp_f32 against exp2f: rounding, not formula.
#                 oracle     float32-seq   kernels' worst (MI355X)   case of the kernels' worst
#   image         6.20e-7    6.15e-7       6.20e-7                   counts-opaque (op level)
#   v_xy          4.68e-7    7.49e-7       1.15e-6                   counts-opaque, tile 2's splats
#   v_conic       4.83e-7    7.97e-7       5.17e-7                   counts-opaque, tile 2's splats
#   v_colors      1.35e-7    7.57e-7       2.01e-7                   counts-opaque, tile 18's splats
#   v_opacity     2.84e-7    1.58e-6       8.46e-7                   counts-opaque, tile 2's splats
#   render        6.67e-6    6.63e-6       7.74e-6                   counts-rgbw (band kernel)
#   loss_abs      3.47e-9    1.27e-6       2.65e-8                   shape-1x1
#   loss_rel      1.23e-8    2.86e-6       4.95e-8                   counts
#   d_xyz         4.87e-5    4.93e-5       6.35e-5                   counts, whole tensor (= tile 2)
#   d_cholesky    3.33e-5    3.31e-5       3.33e-5                   counts, whole tensor (= tile 19)
#   d_features    6.55e-6    6.74e-6       4.28e-6                   counts-L1, tile 2's splat
#   d_rgb_W       1.39e-5    1.39e-5       1.39e-5                   counts-rgbw, tile 19's splat
# (the fused figures are the one-entry tiles' of `counts`: colour up to 20 and a
# centre near x = 70, where float32 spaces 7.6e-6 px -- input rounding that both
# restatements and the kernels share; every other fused case stays below 5e-6.
# `image` is image_error: |d| / max(1, |ref|).  `saturated`'s render goes against
# the C oracle at BARS + WORST, the triangle inequality.)
WORST = dict(image=6.20e-07, v_xy=7.49e-07, v_conic=7.97e-07, v_colors=7.57e-07, v_opacity=1.58e-06,
             render=6.67e-06, loss_abs=1.27e-06, loss_rel=2.86e-06, d_xyz=4.93e-05,
             d_cholesky=3.33e-05, d_features=6.74e-06, d_rgb_W=1.39e-05)
BARS = {k: 4.0 * v for k, v in WORST.items()}
# The tile grids of tests/grid_cases.py (frames of 400x336, 2059x1031 and
# 2059x2040) by the same rule, kept apart so that the bars above stay what they
# were for the cases above: at x ~ 2050 float32 spaces a centre by 2.4e-4 px and
# tanh(xyz) by 6e-8 of a 1030 px half width -- input rounding the float64
# reference does not share, 30 times that of x ~ 70 -- under colours up to 20.
# The op-level image (float32 centres taken as the inputs) and both losses
# (float32 inside a tile, float64 across tiles: publish_loss's summation) stay
# inside WORST; the quantities below do not:
#                 oracle     float32-seq   case of the worse   kernels' worst (MI355X)
#   render        2.48e-4    4.14e-4       grid-R1             2.49e-4 (grid-R1, every path)
#   d_xyz         4.16e-3    5.62e-3       grid-R1-L1          4.23e-3 (grid-R1-L1, tile 5831's splat)
#   d_cholesky    8.10e-4    1.33e-3       grid-R1             8.10e-4 (grid-R1, tile 8255's splat)
#   d_features    1.32e-4    9.84e-5       grid-R2             1.22e-4 (grid-R1, tile 4441's splat)
# (each gradient with the per-tile measure on, over the grids the fused step
# runs on; a tile dropped, stale or run twice is an error of order 1 in its own
# tile's measure and in the render).
WORST_GRID = dict(render=4.14e-04, d_xyz=5.62e-03, d_cholesky=1.33e-03, d_features=1.32e-04)
GRID_BARS = {k: 4.0 * max(v, WORST_GRID.get(k, 0.0)) for k, v in WORST.items()}
OP_GRADS = ("v_xy", "v_conic", "v_colors", "v_opacity")
PARAM_GRADS = (("d_xyz", slice(0, 2)), ("d_cholesky", slice(2, 5)), ("d_features", slice(5, 8)),
               ("d_rgb_W", slice(8, 9)))


# ---------------------------------------------------------------- the rasteriser, any format
def _acc(x, axis, seq):
    """Sum along `axis`: numpy's pairwise sum, or (seq) strictly in index order
    in x's own format."""
    if not seq:
        return x.sum(axis)
    if x.shape[axis] == 0:
        return np.zeros(np.delete(x.shape, axis), x.dtype)
    return np.take(np.cumsum(x, axis=axis, dtype=x.dtype), -1, axis=axis)


def raster_np(c, xy, con, col, op, dt=F64, seq=False):
    """forward.cu:512-627 per tile over its first 256 list entries: a pair is
    kept unless sigma < 0 or alpha = min(1, o e^-sigma) < 1/255; out = sum of
    colour alpha over the kept pairs; final_idx = the last kept list position, 0
    if none.  Also `borderline` (a pixel with a pair within a relative 1e-4 of
    the alpha threshold or |sigma| < 1e-6), the pair counts, and per tile the
    kept mask [pixels, entries] with the terms the backward needs."""
    H, W, f = c["H"], c["W"], dt
    out = np.zeros((H, W, 3), dt)
    idx = np.zeros((H, W), I32)
    border = np.zeros((H, W), bool)
    covered = np.zeros((H, W), bool)
    tiles, pairs, kept, bpairs = [], 0, 0, []
    with np.errstate(over="ignore", invalid="ignore"):
        for t, ii, jj, r0, r1 in _tiles(c):
            g = c["gids"][r0:min(r1, r0 + TILE_PIX)].astype(np.int64)
            K = g.size
            if K == 0:  # an empty tile: nothing to decide or sum (the grids of grid_cases.py have thousands)
                e = np.zeros((ii.size, 0), dt)
                tiles.append(dict(t=t, ii=ii, jj=jj, g=g, dx=e, dy=e, vis=e, w=e, keep=e.astype(bool)))
                continue
            dx = xy[g, 0][None, :] - jj.astype(dt)[:, None]
            dy = xy[g, 1][None, :] - ii.astype(dt)[:, None]
            a, b, cc = con[g, 0][None, :], con[g, 1][None, :], con[g, 2][None, :]
            s = f(0.5) * (a * dx * dx + cc * dy * dy) + b * dx * dy
            vis = np.exp(-s)
            al = np.minimum(f(1.0), op[g][None, :] * vis)
            keep = ~(s < 0) & ~(al < f(ALPHA_MIN))
            bd = (np.abs(al * f(255.0) - f(1.0)) < MARGIN) | (np.abs(s) < SIGMA_MARGIN)
            w = np.where(keep, al, f(0.0)).astype(dt)
            out[ii, jj] = _acc(w[:, :, None] * col[g][None, :, :], 1, seq)
            if K:
                anyk = keep.any(1)
                idx[ii, jj] = np.where(anyk, r0 + K - 1 - np.argmax(keep[:, ::-1], 1), 0)
                border[ii, jj] = bd.any(1)
                covered[ii, jj] = anyk
                bpairs += [(t, int(g[k]), int(ii[p]), int(jj[p])) for p, k in zip(*np.nonzero(bd))]
            pairs += keep.size
            kept += int(keep.sum())
            tiles.append(dict(t=t, ii=ii, jj=jj, g=g, dx=dx, dy=dy, vis=vis, w=w, keep=keep))
    return dict(out=out, idx=idx, borderline=border, covered=covered, tiles=tiles, pairs=pairs,
                kept=kept, border_pairs=bpairs)


def raster_bwd_np(c, fwd, con, col, op, v_out, dt=F64, seq=False):
    """backward.cu:811-858 summed per splat over the kept pairs (an entry past
    a pixel's final_idx is not kept): [N, 9] = v_xy, v_conic (cross term 1/2
    v_sigma dx dy), v_colors, v_opacity."""
    f = dt
    G = np.zeros((c["xys"].shape[0], 9), dt)
    with np.errstate(over="ignore", invalid="ignore"):
        for T in fwd["tiles"]:
            g, keep = T["g"], T["keep"]
            if not keep.any():
                continue
            vo = v_out[T["ii"], T["jj"]].astype(dt)
            cg = col[g]
            z = f(0.0)
            v_al = (vo[:, 0:1] * cg[:, 0][None, :] + vo[:, 1:2] * cg[:, 1][None, :]
                    + vo[:, 2:3] * cg[:, 2][None, :])
            v_s = np.where(keep, -(op[g][None, :] * T["vis"]) * v_al, z)
            dx, dy, w = T["dx"], T["dy"], T["w"]
            a, b, cc = con[g, 0][None, :], con[g, 1][None, :], con[g, 2][None, :]
            hs = f(0.5) * v_s
            cols = (v_s * (a * dx + b * dy), v_s * (b * dx + cc * dy), hs * dx * dx, hs * dx * dy,
                    hs * dy * dy, w * vo[:, 0:1], w * vo[:, 1:2], w * vo[:, 2:3],
                    np.where(keep, T["vis"] * v_al, z))
            for k, x in enumerate(cols):
                G[g, k] += _acc(x.astype(dt), 0, seq)
    return G


def _split_op(G):
    return dict(v_xy=G[:, 0:2], v_conic=G[:, 2:5], v_colors=G[:, 5:8], v_opacity=G[:, 8:9])


def _geo(c, dt=F64):
    return (c["xys"].astype(dt), c["conics"].astype(dt), c["colors"].astype(dt),
            c["opacity"].astype(dt).reshape(-1))


def sum_forward64(c):
    """The float64 sum forward of an op-level case (raster_np)."""
    return raster_np(c, *_geo(c))


def sum_backward64_formula(c, fwd, v_out, dt=F64, seq=False):
    """backward.cu's sums written out (raster_bwd_np) on `fwd`'s decisions."""
    _, con, col, op = _geo(c, dt)
    return _split_op(raster_bwd_np(c, fwd, con, col, op, np.asarray(v_out), dt, seq))


def _raster_torch(c, fwd, xy, con, col, op):
    """The forward as a torch float64 graph with `fwd`'s kept masks fixed and
    the min(1, .) clamp taken straight through (the reference's backward)."""
    out = torch.zeros((c["H"], c["W"], 3), dtype=torch.float64)
    for T in fwd["tiles"]:
        if not T["keep"].any():
            continue
        g, keep = torch.from_numpy(T["g"]), torch.from_numpy(T["keep"])
        ii, jj = torch.from_numpy(T["ii"]), torch.from_numpy(T["jj"])
        dx = xy[g, 0][None, :] - jj.double()[:, None]
        dy = xy[g, 1][None, :] - ii.double()[:, None]
        s = 0.5 * (con[g, 0] * dx * dx + con[g, 2] * dy * dy) + con[g, 1] * dx * dy
        raw = op[g] * torch.exp(-torch.where(keep, s, torch.zeros_like(s)))
        al = raw + (raw.clamp(max=1.0) - raw).detach()
        out = out.index_put((ii, jj), torch.where(keep, al, torch.zeros_like(al)) @ col[g])
    return out


def sum_backward64(c, fwd, v_out):
    """Autograd of the float64 forward with the decisions fixed to `fwd`'s,
    loss = sum out v_out; the v_conic cross term halved (the reference's 1/2
    v_sigma dx dy).  Entries after a pixel's final_idx are not kept: nothing."""
    xy, con, col, op = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in _geo(c))
    loss = (_raster_torch(c, fwd, xy, con, col, op) * torch.tensor(v_out, dtype=torch.float64)).sum()
    if loss.requires_grad:
        loss.backward()
    z = lambda p: np.zeros(tuple(p.shape)) if p.grad is None else p.grad.numpy().copy()  # noqa: E731
    g_con = z(con)
    g_con[:, 1] *= 0.5
    return dict(v_xy=z(xy), v_conic=g_con, v_colors=z(col), v_opacity=z(op).reshape(-1, 1))


# ---------------------------------------------------------------- the training chain, any format
def project_np(means, L, H, W, dt=F64):
    """foward2d.cu:12-69 with helpers.cuh's compute_cov2d_bounds and
    get_tile_bbox: centre (m + 1) size / 2, covariance L L^T, conic, radius =
    ceil(3 sqrt(lambda_max)) with the 0.1 floor on the discriminant, the tile
    box.  Also the margins of the radius and box decisions."""
    f = dt
    tbx, tby = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    hw, hh = f(0.5) * f(W), f(0.5) * f(H)
    cx, cy = hw * means[:, 0] + hw, hh * means[:, 1] + hh
    l11, l21, l22 = L[:, 0], L[:, 1], L[:, 2]
    cxx, cxy, cyy = l11 * l11, l11 * l21, l21 * l21 + l22 * l22
    det = cxx * cyy - cxy * cxy
    ok = det != 0
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(ok, f(1.0) / np.where(ok, det, f(1.0)), f(0.0)).astype(dt)
    conic = np.stack([cyy * inv, -cxy * inv, cxx * inv], 1).astype(dt)
    b = f(0.5) * (cxx + cyy)
    r3 = f(3.0) * np.sqrt(b + np.sqrt(np.maximum(f(0.1), b * b - det)))
    radius = np.where(ok, np.ceil(r3), 0).astype(np.int64)
    m_radius = np.where(ok, np.abs(r3 - np.round(r3)) / r3, np.inf)
    box = np.zeros((means.shape[0], 4), np.int64)
    m_box = np.full(means.shape[0], np.inf)
    rr = radius.astype(dt)
    for k, (v, tb) in enumerate([(cx / f(16) - rr / f(16), tbx), ((cx / f(16) + rr / f(16)) + f(1), tbx),
                                 (cy / f(16) - rr / f(16), tby), ((cy / f(16) + rr / f(16)) + f(1), tby)]):
        box[:, k] = np.clip(np.trunc(v), 0, tb).astype(np.int64)
        near = np.round(v)  # the decision matters only where int(v) lands in 1..tb
        m = np.where((near >= 1) & (near <= tb), np.abs(v - near) / np.maximum(1.0, np.abs(v)), np.inf)
        m_box = np.minimum(m_box, np.where(ok, m, np.inf))
    box[~ok] = 0
    xy = np.where(ok[:, None], np.stack([cx, cy], 1), f(0.0)).astype(dt)
    return dict(xy=xy, conic=conic, radius=radius, box=box, ok=ok, m_radius=m_radius, m_box=m_box)


def bin_np(box, tbx, tby):
    """The tile lists in (tile, id) order (depth is 0: utils.py:121-167)."""
    lists = [[] for _ in range(tbx * tby)]
    area = (box[:, 1] - box[:, 0]) * (box[:, 3] - box[:, 2])
    for i in np.flatnonzero(area > 0):
        x0, x1, y0, y1 = box[i]
        for y in range(y0, y1):
            for x in range(x0, x1):
                lists[y * tbx + x].append(i)
    return [np.asarray(l, I32) for l in lists]


def chain_np(p, dt=F64, seq=False):
    """GaussianSplats_Represent.py:57-70,191-195 from the raw parameters: tanh,
    + bound, * rgb_W; projection; binning; the sum forward; clamp; L2 or L1
    loss; its gradient through the clamp (torch's rule: it passes where 0 <=
    out <= 1), the rasteriser, the projection (backward2d.cu, the L cross term
    doubled as there) and the activations.  M < 1: the image is the clamped
    background and nothing flows.  Returns the clamped render [3, H, W], (mse,
    l1), grads [N, 9] (d_xyz, d_cholesky, d_features, d_rgb_W), the geometry
    and every decision's margin."""
    f, H, W = dt, p["H"], p["W"]
    n = p["xyz"].shape[0]
    tbx, tby = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    xyz, chol, feat, rgbw = (p[k].astype(dt) for k in ("xyz", "chol", "feat", "rgbw"))
    means = np.tanh(xyz.astype(F64)).astype(dt)  # (float32: correctly rounded, whatever the CPU's SIMD tanh)
    L = chol + p["bound"].astype(dt)[None, :]
    colors = feat * rgbw
    pr = project_np(means, L, H, W, dt)
    lists = bin_np(pr["box"], tbx, tby)
    c = _set_lists(dict(H=H, W=W, xys=pr["xy"]), lists)
    gt = p["gt"].astype(dt).reshape(3, H, W)
    numel = 3 * H * W
    res = dict(c=c, proj=pr, means=means, L=L, colors=colors, M=int(c["counts"].sum()))

    def losses(img):
        d = img - gt
        flat = d.reshape(-1)
        return d, (float(_acc(flat * flat, 0, seq)) / numel, float(_acc(np.abs(flat), 0, seq)) / numel)

    if res["M"] < 1:
        img = np.broadcast_to(np.clip(p["bg"].astype(dt), 0, 1)[:, None, None], (3, H, W)).astype(dt)
        res.update(render=img, losses=losses(img)[1], grads=np.zeros((n, 9), dt), fwd=None,
                   margins=dict(cut=np.inf, sigma=np.inf, clamp=np.inf, absd=np.inf,
                                radius=float(pr["m_radius"].min()), box=float(pr["m_box"].min())))
        return res
    op = np.ones(n, dt)
    fwd = raster_np(c, pr["xy"], pr["conic"], colors, op, dt, seq)
    out = fwd["out"]
    passes = (out >= 0) & (out <= 1)
    img = np.clip(out, f(0.0), f(1.0)).transpose(2, 0, 1)
    d, ls = losses(img)
    v_img = (f(2.0) / f(numel)) * d if p["loss"] == "L2" else np.sign(d) / f(numel)
    v_out = np.where(passes, v_img.transpose(1, 2, 0), f(0.0)).astype(dt)
    G = raster_bwd_np(c, fwd, pr["conic"], colors, op, v_out, dt, seq)
    # backward2d.cu:8-51 with cov2d_to_conic_vjp: v_cov = -X G X, G01 = G10 = v_conic.y
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
    grads[:, 2] = two * l11 * g11 + two * g12 * l21  # the reference's doubled cross term
    grads[:, 3] = two * l11 * g12 + two * l21 * g22
    grads[:, 4] = two * l22 * g22
    grads[:, 5:8] = G[:, 5:8] * rgbw
    if p["rgbw_train"]:
        grads[:, 8] = (G[:, 5] * feat[:, 0] + G[:, 6] * feat[:, 1]) + G[:, 7] * feat[:, 2]
    grads[~pr["ok"]] = 0
    # margins of the decisions a gradient depends on
    live = fwd["covered"][:, :, None] & np.ones(3, bool)
    cl = np.minimum(np.abs(out), np.abs(out - 1))[live]
    dd = np.abs(d.transpose(1, 2, 0))[live & passes]
    mc, ms = np.inf, np.inf
    for T in fwd["tiles"]:
        if T["g"].size:
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                s = -np.log(T["vis"])
                mc = min(mc, float(np.nanmin(np.abs(np.minimum(1.0, T["vis"]) * 255.0 - 1.0))))
                ms = min(ms, float(np.nanmin(np.abs(s))))
    res.update(render=img, losses=ls, grads=grads, fwd=fwd, out=out, passes=passes, v_out=v_out, d=d,
               margins=dict(cut=mc, sigma=ms, clamp=float(cl.min()) if cl.size else np.inf,
                            absd=(float(dd.min()) if dd.size else np.inf) if p["loss"] == "L1" else np.inf,
                            radius=float(pr["m_radius"].min()), box=float(pr["m_box"].min())))
    return res


MARGIN_FLOOR = dict(cut=MARGIN, sigma=SIGMA_MARGIN, clamp=CLAMP_MARGIN, absd=CLAMP_MARGIN,
                    radius=MARGIN, box=MARGIN)


def train_grads64(p):
    """The float64 reference of a fused-step case (chain_np in float64)."""
    return chain_np(p, F64, False)


def train_grads64_autograd(p, ref):
    """torch float64 autograd from the raw parameters through tanh, + bound,
    * rgb_W, the projection, the forward (`ref`'s lists and decisions fixed),
    torch.clamp and F.mse_loss / F.l1_loss; the Cholesky gradient gets the
    reference's doubled cross term from the retained covariance gradient.
    Returns (render [3, H, W], loss, grads [N, 9])."""
    H, W = p["H"], p["W"]
    n = p["xyz"].shape[0]
    t = lambda a: torch.tensor(np.asarray(a, F64), dtype=torch.float64)  # noqa: E731
    xyz, chol, feat, rgbw = (t(p[k]).requires_grad_(True) for k in ("xyz", "chol", "feat", "rgbw"))
    if ref["M"] < 1:
        return ref["render"], ref["losses"], np.zeros((n, 9))
    ok = torch.from_numpy(ref["proj"]["ok"])
    means = torch.tanh(xyz)
    L = chol + t(p["bound"])[None, :]
    colors = feat * rgbw
    xy = torch.stack([0.5 * W * means[:, 0] + 0.5 * W, 0.5 * H * means[:, 1] + 0.5 * H], 1)
    cxx, cxy, cyy = L[:, 0] * L[:, 0], L[:, 0] * L[:, 1], L[:, 1] * L[:, 1] + L[:, 2] * L[:, 2]
    cxy.retain_grad()
    det = torch.where(ok, cxx * cyy - cxy * cxy, torch.ones_like(cxx))
    con = torch.stack([cyy / det, -cxy / det, cxx / det], 1)
    out = _raster_torch(ref["c"], ref["fwd"], xy, con, colors, torch.ones(n, dtype=torch.float64))
    img = torch.clamp(out, 0, 1).permute(2, 0, 1)
    gt = t(p["gt"]).reshape(3, H, W)
    F = torch.nn.functional
    loss = F.mse_loss(img, gt) if p["loss"] == "L2" else F.l1_loss(img, gt)
    loss.backward()
    g12 = cxy.grad
    gl = chol.grad.clone()
    gl[:, 0] += g12 * L[:, 1].detach()
    gl[:, 1] += g12 * L[:, 0].detach()
    grads = torch.cat([xyz.grad, gl, feat.grad, rgbw.grad if p["rgbw_train"] else torch.zeros(n, 1,
                      dtype=torch.float64)], 1)
    grads[~ok] = 0
    return img.detach().numpy(), loss.item(), grads.numpy()


# ---------------------------------------------------------------- op-level cases
SUM_COUNTS = [257, 0, 1, 7, 8, 9, 24, 25, 63, 64, 65, 96, 97, 128, 129, 0, 300, 255, 256, 1]
REUSED = (["shape-1x1", "shape-1x37", "shape-37x1", "shape-5x3", "shape-15x17", "shape-17x15",
           "shape-33x18", "shape-20x70", "shape-37x45"]
          + ["blockedge", "nine-tiles", "noblend", "opacities", "counts-faint", "counts-opaque"])
OP_IDS = REUSED + ["counts-sum"]
OP_COUNT_IDS = ["counts-faint", "counts-opaque", "counts-sum"]
NUDGE = np.array([0.0037, -0.0029], F32)
_op_cache = {}


def _sum_count_case():
    """50x70 (4 x 5 tiles, both edges partial), per-tile counts SUM_COUNTS: the
    switches of raster_sum.hip (kHeadSlots 8, kGroupMinDefault 24 | 25, kChunk
    64, kDenseEntriesPerTile 96 | 97, kSBChunk remainders, 128 | 129, 255 | 256 |
    257 | 300), empty tiles next to the fullest; the tiles past 256 are the
    first tile and a bottom (two-row) one."""
    c = _frame(50, 70, 900, 43, opac=(0.05, 0.9))
    _set_lists(c, [_nearest(c, t, k) for t, k in enumerate(SUM_COUNTS)])
    c.update(id="counts-sum", path="raster_sum.hip list / chunk switches, the 256-entry cut")
    c["claims"]["counts"] = SUM_COUNTS
    return c


def op_case(cid):
    """An op-level case: alpha_cases' geometry (or the sum-only counts case),
    copied, with every splat that has a borderline pair nudged by a few
    thousandths of a pixel until no (entry, pixel) decision of the case lies
    within its margin; the float64 forward and both gradient statements' inputs
    are cached with it."""
    if cid not in _op_cache:
        src = _sum_count_case() if cid == "counts-sum" else A.BY_ID[cid]
        c = dict(src)
        c["xys"] = src["xys"].copy()
        c["nudged"] = 0
        for _ in range(40):
            fwd = sum_forward64(c)
            bad = sorted({g for _, g, _, _ in fwd["border_pairs"]})
            if not bad:
                break
            c["xys"][bad] += NUDGE
            c["nudged"] += len(bad)
        c["fwd"] = fwd
        _op_cache[cid] = c
    return _op_cache[cid]


def op_reference(cid):
    c = op_case(cid)
    if "ref" not in c:
        c["ref"] = sum_backward64(c, c["fwd"], c["v_out"])
    return c["fwd"], c["ref"]


def truncated(c):
    """The case with every tile's list cut to its first 256 entries."""
    t = dict(c)
    return _set_lists(t, [c["gids"][r0:min(r1, r0 + TILE_PIX)] for r0, r1 in c["bins"]])


def only_past_256(c):
    """Splats that some tile lists past its 256th entry and no tile lists
    before it: their gradient rows are exactly zero."""
    n = c["xys"].shape[0]
    live, late = np.zeros(n, bool), np.zeros(n, bool)
    for r0, r1 in c["bins"]:
        live[c["gids"][r0:min(r1, r0 + TILE_PIX)]] = True
        late[c["gids"][min(r1, r0 + TILE_PIX):r1]] = True
    return late & ~live


# ---------------------------------------------------------------- fused-step cases
COUNTS = [257, 0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 300, 0, 257, 64, 65, 1]
SHAPES = [(1, 1), (1, 37), (37, 1), (17, 15), (15, 17), (33, 18), (37, 45)]
FUSED_IDS = (["counts", "counts-L1", "counts-rgbw", "span", "span-L1"]
             + [f"shape-{h}x{w}" for h, w in SHAPES] + ["id-window", "saturated", "empty"])
FUSED_COUNT_IDS = ["counts", "counts-L1", "counts-rgbw"]
_fused_cache = {}


def _radius64(L):
    l11, l21, l22 = (np.asarray(L, F64)[..., k] for k in range(3))
    cxx, cyy, det = l11 * l11, l21 * l21 + l22 * l22, (l11 * l22) ** 2
    b = 0.5 * (cxx + cyy)
    return 3.0 * np.sqrt(b + np.sqrt(np.maximum(0.1, b * b - det)))


def _small_L(rng, k):
    """k Cholesky rows with l11, l22 in [0.55, 0.95], |l21| <= 0.3, redrawn
    while 3 sqrt(lambda) is within 1e-3 of an integer (the radius decision)."""
    L = np.zeros((k, 3), F32)
    todo = np.arange(k)
    while todo.size:
        L[todo] = np.stack([rng.uniform(0.55, 0.95, todo.size), rng.uniform(-0.3, 0.3, todo.size),
                            rng.uniform(0.55, 0.95, todo.size)], 1).astype(F32)
        r3 = _radius64(L[todo])
        todo = todo[np.abs(r3 - np.round(r3)) < 1e-3 * r3]
    return L


def _one_tile_centres(rng, t, L, H, W):
    """Centres for the splats L inside tile t, at least radius + 0.1 px from the
    lines the tile shares with a neighbour and inside the image, so that each
    splat's tile box is tile t alone."""
    tbx, tby = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    ty, tx = divmod(t, tbx)
    r = np.ceil(_radius64(L)) + 0.1
    k = L.shape[0]
    x_lo = np.where(tx > 0, tx * TILE + r, 0.3)
    x_hi = np.where(tx < tbx - 1, (tx + 1) * TILE - r, W - 0.3)
    y_lo = np.where(ty > 0, ty * TILE + r, 0.3)
    y_hi = np.where(ty < tby - 1, (ty + 1) * TILE - r, H - 0.3)
    assert (x_lo < x_hi).all() and (y_lo < y_hi).all()
    return np.stack([rng.uniform(x_lo, x_hi, k), rng.uniform(y_lo, y_hi, k)], 1)


def _raw_xyz(centres, H, W):
    m = 2.0 * np.asarray(centres, F64) / np.array([W, H], F64) - 1.0
    return np.arctanh(m).astype(F32)


def _params(H, W, xyz, L, feat, seed, loss="L2", rgbw=None, rgbw_train=False, bg=(1.0, 1.0, 1.0)):
    rng = np.random.default_rng(seed + 1000)
    n = xyz.shape[0]
    return dict(H=H, W=W, xyz=np.asarray(xyz, F32), chol=(np.asarray(L, F32) - BOUND).astype(F32),
                feat=np.asarray(feat, F32), rgbw=np.ones((n, 1), F32) if rgbw is None else rgbw,
                rgbw_train=rgbw_train, bound=BOUND.copy(), bg=np.asarray(bg, F32), loss=loss,
                gt=rng.random((3, H, W)).astype(F32), claims={})


def _counts_frame(seed, extra=0):
    """58x74 (4 x 5 tiles; the bottom tiles hold 10 rows, the right tiles 10
    columns), per-tile counts COUNTS from placement: small splats, one tile
    each, ids shuffled; colours U(-0.3, 1) 20 / k in a tile of k.  extra: that
    many larger splats (the small shapes x 4..8) across bands, tiles and the
    image edges, faint colours, appended to the id range before the shuffle."""
    H, W = 58, 74
    rng = np.random.default_rng(seed)
    Ls, cs, cols, tile_of = [], [], [], []
    for t, k in enumerate(COUNTS):
        if k == 0:
            continue
        L = _small_L(rng, k)
        Ls.append(L)
        cs.append(_one_tile_centres(rng, t, L, H, W))
        cols.append(rng.uniform(-0.3, 1.0, (k, 3)) * 20.0 / k)
        tile_of += [t] * k
    if extra:
        L = _small_L(rng, extra) * rng.uniform(4.0, 8.0, (extra, 1)).astype(F32)
        Ls.append(L)
        cs.append(np.stack([rng.uniform(1.0, W - 1.0, extra), rng.uniform(1.0, H - 1.0, extra)], 1))
        cols.append(rng.uniform(-0.3, 1.0, (extra, 3)) * 0.02)
        tile_of += [-1] * extra
    L, centres, col = np.concatenate(Ls), np.concatenate(cs), np.concatenate(cols)
    perm = rng.permutation(L.shape[0])
    return H, W, L[perm], centres[perm], col[perm].astype(F32), np.asarray(tile_of)[perm]


def _build_fused(cid):
    if cid.startswith("counts") or cid.startswith("span"):
        span = cid.startswith("span")
        H, W, L, centres, col, tile_of = _counts_frame(7 if span else 5, extra=40 if span else 0)
        kw = dict(loss="L1" if cid.endswith("L1") else "L2")
        if cid == "counts-rgbw":
            w = np.random.default_rng(3).uniform(0.5, 1.5, (L.shape[0], 1)).astype(F32)
            kw.update(rgbw=w, rgbw_train=True)
            col = (col / w).astype(F32)
        p = _params(H, W, _raw_xyz(centres, H, W), L, col, 31, **kw)
        p["claims"].update(tile_of=tile_of, counts=COUNTS)
        return p
    if cid.startswith("shape-"):
        H, W = (int(v) for v in cid[6:].split("x"))
        rng = np.random.default_rng(100 + H * 64 + W)
        n = max(16, int(0.075 * (H + 8) * (W + 8)))
        xyz = np.arctanh(rng.uniform(-0.999, 0.999, (n, 2))).astype(F32)
        L = (rng.random((n, 3)) + np.array([0.5, 0.0, 0.5])).astype(F32)
        per_pixel = max(1.0, n * 25.0 / (H * W))
        return _params(H, W, xyz, L, rng.uniform(-0.3, 1.0, (n, 3)) * 1.5 / per_pixel, 41)
    if cid == "id-window":
        H, W, n = 64, 64, 40001
        rng = np.random.default_rng(17)
        ids_a = np.concatenate([[5, 40000], rng.choice(np.arange(6, 40000), 128, replace=False)])
        ids_b = 17000 + rng.choice(np.setdiff1d(np.arange(3000), ids_a - 17000), 70, replace=False)
        assert np.unique(np.concatenate([ids_a, ids_b])).size == 200
        xyz = np.zeros((n, 2), F32)
        L = np.zeros((n, 3), F32)  # _cholesky = -bound: det = 0, skipped
        feat = rng.uniform(-0.3, 1.0, (n, 3))
        for ids, t in ((ids_a, 5), (ids_b, 10)):
            Lk = _small_L(rng, ids.size)
            L[ids] = Lk
            xyz[ids] = _raw_xyz(_one_tile_centres(rng, t, Lk, H, W), H, W)
            feat[ids] *= 20.0 / ids.size
        p = _params(H, W, xyz, L, feat, 51)
        p["claims"].update(ids_a=np.sort(ids_a), ids_b=np.sort(ids_b), tiles=(5, 10))
        return p
    if cid == "saturated":
        H, W, n = 64, 48, 160
        rng = np.random.default_rng(23)
        xyz = np.arctanh(rng.uniform(-0.97, 0.97, (n, 2))).astype(F32)
        L = (rng.random((n, 3)) + np.array([0.5, 0.0, 0.5])).astype(F32)
        sat = [(9, 0.3), (-9, -0.2), (0.1, 9), (0.4, -9), (20, 20), (-20, 20), (20, -20), (-20, -2.5),
               (20, 0.7), (-0.6, -20), (9, 9), (-9, 20)]
        xyz[:len(sat)] = np.array(sat, F32)
        k = len(sat)
        # centres in the last half pixel of the right / bottom edge
        xyz[k:k + 8, 0] = _raw_xyz(np.stack([W - rng.uniform(0.02, 0.5, 8), np.ones(8)], 1), H, W)[:, 0]
        xyz[k + 8:k + 16, 1] = _raw_xyz(np.stack([np.ones(8), H - rng.uniform(0.02, 0.5, 8)], 1), H, W)[:, 1]
        p = _params(H, W, xyz, L, rng.uniform(-0.3, 1.0, (n, 3)) * 0.6, 61)
        p["claims"].update(saturated=np.arange(len(sat)), last_half=np.arange(k, k + 16))
        return p
    if cid == "empty":
        H, W, n = 40, 56, 300
        rng = np.random.default_rng(29)
        xyz = np.arctanh(rng.uniform(-0.99, 0.99, (n, 2))).astype(F32)
        return _params(H, W, xyz, np.zeros((n, 3), F32), rng.random((n, 3)), 71, bg=(0.25, 1.5, -0.5))
    if cid in _extra_builders:
        return _extra_builders[cid](cid)
    raise KeyError(cid)


_extra_builders = {}


def register_fused(cid, builder):
    """A fused-step case built elsewhere (tests/grid_cases.py): fused_case runs
    builder(cid) through the same nudging loop and caches it the same way."""
    assert cid not in FUSED_IDS
    _extra_builders[cid] = builder


def _offenders(p, r):
    """What lies behind the decisions of `r` within their margin: splats to
    move (the cut, a radius, a tile box), splats to recolour (a clamped value
    within 1e-5 of 0 or 1: the pixel's strongest contributor) and target
    elements to move (|d| < 1e-5 under L1)."""
    pr, fwd = r["proj"], r["fwd"]
    move = set(np.flatnonzero((pr["m_radius"] < MARGIN) | (pr["m_box"] < MARGIN)).tolist())
    recolour, gt_fix = set(), []
    if fwd is not None:
        move |= {g for _, g, _, _ in fwd["border_pairs"]}
        out, live = r["out"], fwd["covered"]
        near = live[:, :, None] & (np.minimum(np.abs(out), np.abs(out - 1)) < CLAMP_MARGIN)
        for i, j, ch in zip(*np.nonzero(near)):
            T = fwd["tiles"][(i // TILE) * ((p["W"] + TILE - 1) // TILE) + j // TILE]
            q = np.flatnonzero((T["ii"] == i) & (T["jj"] == j))[0]
            recolour.add((int(T["g"][np.argmax(T["w"][q])]), int(ch)))
        if p["loss"] == "L1":
            dd = np.abs(r["d"]) < CLAMP_MARGIN
            gt_fix = list(zip(*np.nonzero(dd & (live[None] & r["passes"].transpose(2, 0, 1)))))
    return sorted(move), sorted(recolour), gt_fix


def fused_case(cid):
    """A fused-step case and its float64 reference.  The builder moves every
    splat behind a cut, radius or box decision within its margin (centre by
    ~1e-3 of the frame; the Cholesky factor by 1e-3 too where the radius or a
    saturated centre is the cause), shifts the colour of the strongest entry behind a clamped value
    within 1e-5 of 0 or 1 (x 1.003 + 0.003), and moves a target element with |d| < 1e-5
    (L1), until the case has no borderline decision; test_sum_cases_cpu.py
    asserts the result."""
    if cid not in _fused_cache:
        p = _build_fused(cid)
        p["id"] = cid
        p["nudged"] = 0
        for it in range(40):
            r = train_grads64(p)
            move, recolour, gt_fix = _offenders(p, r)
            if not move and not recolour and not gt_fix:
                break
            step = F32(1e-3 * (1 + it % 3))
            p["xyz"][move] += np.array([step, -0.7 * step], F32)
            stuck = [g for g in move if r["proj"]["m_radius"][g] < MARGIN or np.abs(p["xyz"][g]).max() > 4]
            p["chol"][stuck] *= F32(1.001)
            for g, ch in recolour:
                p["feat"][g, ch] = F32(1.003) * p["feat"][g, ch] + F32(0.003)
            for k in gt_fix:
                p["gt"][k] = F32(0.5 * p["gt"][k] + 0.2)
            p["nudged"] += len(move) + len(recolour) + len(gt_fix)
        else:
            raise AssertionError(f"{cid}: decisions within their margin remain: {r['margins']}")
        _fused_cache[cid] = (p, r)
    return _fused_cache[cid]


def activated32(p):
    """float32 activations of a case (tanh correctly rounded: float64's,
    rounded once): the C oracle's inputs."""
    return (np.tanh(p["xyz"].astype(F64)).astype(F32), (p["chol"] + p["bound"]).astype(F32),
            (p["feat"] * p["rgbw"]).astype(F32))


# ---------------------------------------------------------------- rectangles of the backward
def rect64(xy, conic, tx0, ty0):
    """rows.h ellipse_rect in float64 for unit opacity: the tile pixels inside
    the alpha >= 1/255 ellipse's bounding box with the kernel's 0.1 % + 0.01 px
    margins, as inclusive (x0, x1, y0, y1) per splat; x0 > x1: none."""
    a, b, cc = conic[:, 0], conic[:, 1], conic[:, 2]
    det = a * cc - b * b
    S2 = 2.0 * (math.log(255.0) * 1.001 + 0.01)
    ex = np.sqrt(S2 * cc / det) * 1.001 + 0.01
    ey = np.sqrt(S2 * a / det) * 1.001 + 0.01
    x0, x1 = np.maximum(np.ceil(xy[:, 0] - ex - tx0), 0), np.minimum(np.floor(xy[:, 0] + ex - tx0), 15)
    y0, y1 = np.maximum(np.ceil(xy[:, 1] - ey - ty0), 0), np.minimum(np.floor(xy[:, 1] + ey - ty0), 15)
    none = ~((x0 <= x1) & (y0 <= y1))
    r = np.stack([x0, x1, y0, y1], 1).astype(np.int64)
    r[none] = (15, 0, 15, 0)
    return r


# ---------------------------------------------------------------- error measures
def listed(c):
    m = np.zeros(c["xys"].shape[0], bool)
    for r0, r1 in c["bins"]:
        m[c["gids"][r0:r1]] = True
    return m


def edge_splats(c):
    """Listed splats centred within EDGE_PX of the right or bottom image edge."""
    xy = c["xys"]
    return listed(c) & ((xy[:, 0] >= c["W"] - 1 - EDGE_PX) | (xy[:, 1] >= c["H"] - 1 - EDGE_PX))


def tile_groups(c):
    """Per non-empty tile, the splats it lists."""
    return [(t, np.unique(c["gids"][r0:r1])) for t, (r0, r1) in enumerate(c["bins"]) if r1 > r0]


def grad_errors(c, got, ref, per_tile=False, rows=None):
    """(whole, edge, tile, worst tile): a gradient tensor's error relative to
    the reference's largest element over the whole tensor, over the edge splats
    relative to that subset's largest, and (per_tile) the worst over the tiles
    of one tile's splats relative to the largest element among them -- the
    measure that can see a dense tile, whose gradients are orders of magnitude
    below a sparse tile's.  rows: restrict every measure to these splats."""
    got, ref = np.asarray(got, F64).reshape(np.shape(ref)), np.asarray(ref, F64)
    sel = np.ones(ref.shape[0], bool) if rows is None else np.asarray(rows)
    e = edge_splats(c) & sel
    whole, edge = rel_error(got[sel], ref[sel]), rel_error(got[e], ref[e])
    worst, where = 0.0, -1
    if per_tile:
        for t, ids in tile_groups(c):
            ids = ids[sel[ids]]
            err = rel_error(got[ids], ref[ids])
            if err > worst:
                worst, where = err, t
    return whole, edge, worst, where


def saturated_rows(p):
    """Splats whose 1 - tanh^2 float64 decides (|xyz| < 4 on both axes)."""
    return np.abs(p["xyz"]).max(1) < 4.0


def image_error(got, ref, keep=None):
    """max |got - ref| / max(1, |ref|): absolute over the range the product
    renders (the clamp's [0, 1]), relative above it -- an unclamped sum of 257
    opaque entries reaches ~100, where float32's own spacing is 8e-6."""
    got, ref = np.asarray(got, F64).reshape(np.shape(ref)), np.asarray(ref, F64)
    err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    return float((err if keep is None else err[keep]).max())


def op_errors(cid, out, idx, grads):
    """An op-level result against the float64 references: the image
    (image_error, off the borderline mask), final_idx mismatches off the mask,
    and per gradient (whole, edge, worst tile, that tile)."""
    c = op_case(cid)
    fwd, ref = op_reference(cid)
    keep = ~fwd["borderline"]
    e = dict(image=image_error(out, fwd["out"], keep),
             idx=int((np.asarray(idx)[keep] != fwd["idx"][keep]).sum()))
    for name, g in zip(OP_GRADS, grads):
        e[name] = grad_errors(c, g, ref[name], per_tile=cid in OP_COUNT_IDS)
    return e


def fused_errors(cid, render, losses, grads, image_ref=None):
    """A fused-step result against train_grads64: the clamped render
    (absolute; against `image_ref` where given), both losses (absolute and
    relative) and per parameter gradient (whole, edge, worst tile, that tile);
    `saturated` compares the gradient rows float64 decides."""
    p, r = fused_case(cid)
    ref_img = r["render"] if image_ref is None else image_ref
    ref_l = np.asarray(r["losses"], F64)
    dl = np.abs(np.asarray(losses, F64)[:2] - ref_l)
    e = dict(render=float(np.abs(np.asarray(render, F64).reshape(ref_img.shape) - ref_img).max()),
             loss_abs=float(dl.max()), loss_rel=float((dl / ref_l).max()))
    rows = saturated_rows(p) if cid == "saturated" else None
    grads = np.asarray(grads, F64)
    for name, sl in PARAM_GRADS:
        e[name] = grad_errors(r["c"], grads[:, sl], r["grads"][:, sl], per_tile=cid in FUSED_COUNT_IDS,
                              rows=rows)
    return e


def worst_of(e, name):
    v = e[name]
    return max(v[:3]) if isinstance(v, tuple) else v


# ---------------------------------------------------------------- the two float32 restatements
def oracle_op(c):
    """The C oracle (float32, sums in double) on an op-level case: image,
    final_idx and the backward on its own final_idx."""
    import oracle as O
    tb = O.tile_bounds(c["H"], c["W"])
    args = (c["gids"], c["bins"], c["xys"], c["conics"], c["colors"], c["opacity"])
    out, _, idx = O.raster_sum_forward(tb, c["H"], c["W"], *args)
    return out, idx, O.raster_sum_backward(tb, c["H"], c["W"], *args, idx, c["v_out"])


def oracle_op_forward(c):
    """The C oracle's image and final_idx of an op-level case."""
    import oracle as O
    out, _, idx = O.raster_sum_forward(O.tile_bounds(c["H"], c["W"]), c["H"], c["W"], c["gids"], c["bins"],
                                       c["xys"], c["conics"], c["colors"], c["opacity"])
    return out, idx


def float32_op_forward(c):
    """raster_np in float32 with sequential float32 sums: image and final_idx."""
    fwd = raster_np(c, *_geo(c, F32), F32, True)
    return fwd["out"], fwd["idx"]


def float32_op(c):
    """raster_np / raster_bwd_np in float32 with sequential float32 sums."""
    fwd = raster_np(c, *_geo(c, F32), F32, True)
    g = sum_backward64_formula(c, fwd, c["v_out"], F32, True)
    return fwd["out"], fwd["idx"], [g[k] for k in OP_GRADS]


def oracle_fused(p):
    """The C oracle's operators chained as GaussianSplats_Represent.py:191-195
    from numpy's float32 activations: (render [3, H, W], (mse, l1), grads
    [N, 9])."""
    import oracle as O
    H, W = p["H"], p["W"]
    n = p["xyz"].shape[0]
    means, L, colors = activated32(p)
    tb = O.tile_bounds(H, W)
    xys, depths, radii, conics, nth = O.project_2d_forward(means, L, H, W, tb)
    m, cum = O.cumulative_intersects(nth)
    gt = p["gt"].reshape(3, H, W)
    numel = 3 * H * W
    grads = np.zeros((n, 9), F32)
    if m < 1:
        img = np.broadcast_to(np.clip(p["bg"], 0, 1)[:, None, None], (3, H, W)).astype(F32)
    else:
        _, _, _, gids, bins = O.bin_and_sort(xys, depths, radii, cum, tb, m)
        opac = np.ones((n, 1), F32)
        out, _, idx = O.raster_sum_forward(tb, H, W, gids, bins, xys, conics, colors, opac)
        img = np.clip(out, 0, 1).transpose(2, 0, 1)
    d = (img - gt).astype(F32)
    losses = (float(np.mean(d.astype(F64) ** 2)), float(np.mean(np.abs(d.astype(F64)))))
    if m >= 1:
        v_img = (F32(2.0 / numel) * d if p["loss"] == "L2" else np.sign(d) * F32(1.0 / numel)).astype(F32)
        v_out = np.where((out >= 0) & (out <= 1), v_img.transpose(1, 2, 0), F32(0)).astype(F32)
        v_xy, v_conic, v_rgb, _ = O.raster_sum_backward(tb, H, W, gids, bins, xys, conics, colors, opac,
                                                       idx, np.ascontiguousarray(v_out))
        _, v_mean, v_L = O.project_2d_backward(L, H, W, radii, conics, v_xy.astype(F32),
                                               v_conic.astype(F32))
        v_rgb = v_rgb.astype(F32)
        grads[:, 0:2] = v_mean * (F32(1) - means * means)
        grads[:, 2:5] = v_L
        grads[:, 5:8] = v_rgb * p["rgbw"]
        if p["rgbw_train"]:
            grads[:, 8] = (v_rgb[:, 0] * p["feat"][:, 0] + v_rgb[:, 1] * p["feat"][:, 1]) \
                + v_rgb[:, 2] * p["feat"][:, 2]
    return img, losses, grads


def float32_fused(p):
    """chain_np in float32 with sequential float32 sums."""
    r = chain_np(p, F32, True)
    return r["render"], r["losses"], r["grads"]
