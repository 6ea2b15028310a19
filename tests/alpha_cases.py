"""Cases, float64 references, error measures and bars shared by
test_alpha_cases_cpu.py (premises, no GPU), test_alpha_edges.py (the HIP
kernels of gsvc_amd/csrc/raster_alpha.hip) and tests/analysis/alpha_bars.py
(where the bars come from).

The references are plain numpy / torch float64 written from the reference's
forward.cu:252-374 and backward.cu:138-315; they import nothing from the code
under test and do not call the C oracle (which only projects and bins the
seeded frames the cases start from).  Two quirks of the reference are kept
and stated, not hidden:

* backward.cu:284-286 gives v_conic.y = 1/2 v_sigma dx dy, HALF the true
  derivative of sigma = 1/2 (a dx^2 + c dy^2) + b dx dy by b (the projection
  backward doubles it again).  `alpha_backward64_autograd` halves its cross
  term to match; `alpha_backward64_recursion` states the halved form.
* the forward clamps alpha at 0.999 and the backward at 0.99 (forward.cu:339,
  backward.cu:244), and the backward lets the gradient through the clamp.
  Where a blended raw alpha exceeds 0.99 the reference's gradient is by design
  not the forward's derivative: such pixels are in the `hi99` mask, autograd is
  valid only where it is empty, the recursion everywhere.

Float64 does not apply to the CALLER cases: a conic that is not positive
definite has sigma < 0 on part of the tile and a needle (a c > 8192 det) has a
float32 sigma that cancels to noise, so which (entry, pixel) pairs blend is a
property of the float32 evaluation order itself, and a NaN colour has no
ordering; those go against the C oracle, which evaluates sigma with the
kernels' own operation order.
"""
import math

import numpy as np
import torch

import oracle as O

F32, F64, I32 = np.float32, np.float64, np.int32
TILE = 16
ALPHA_MIN = 1.0 / 255.0
T_STOP = 1e-4
MARGIN = 1e-4        # relative distance of a decision from its threshold: borderline
SIGMA_MARGIN = 1e-6  # |sigma| below this: the sigma < 0 test is borderline
EDGE_PX = 4.0        # splats centred within this of the right / bottom edge: the edge subset

# ---------------------------------------------------------------- bars
# 4 x the C oracle's (the float32 restatement's) worst error against float64
# over CASES, per quantity (tests/analysis/alpha_bars.py prints them): image and
# T absolute, each gradient relative to the reference's largest element, the
# worse of the whole tensor and the edge subset.  The margin covers the
# kernels' other summation tree (DPP row sums, float atomics) and the hardware
# reciprocal: rounding, not formula.
#              oracle worst (CPU)   kernels' worst (MI355X)   case of the kernels' worst
#   image          4.23e-7              1.23e-7               shape-37x45 (through the glue)
#   T              1.56e-7              1.55e-7               shape-17x15
#   v_xy           7.50e-7              9.50e-7               counts-opaque, v_out alone, edge subset
#   v_conic        8.70e-7              6.74e-7               nine-tiles
#   v_colors       2.79e-6              2.80e-6               clamp-99, edge subset
#   v_opacity      1.24e-6              1.18e-6               clamp-99
# (the oracle's worst image error is counts-opaque's; the backward's spread
# over three calls stays below 1.4e-7 of the largest element, nine-tiles.)
WORST = dict(image=4.23e-7, T=1.56e-7, v_xy=7.50e-7, v_conic=8.70e-7, v_colors=2.79e-6,
             v_opacity=1.24e-6)
BARS = {k: 4.0 * v for k, v in WORST.items()}
GRADS = ("v_xy", "v_conic", "v_colors", "v_opacity")


# ---------------------------------------------------------------- building cases
def _ntiles(H, W):
    return ((W + TILE - 1) // TILE) * ((H + TILE - 1) // TILE)


def _frame(H, W, n, seed, opac=(0.05, 0.9), chol=1.0, margin_px=4.0, pin=None):
    """A seeded frame projected and binned by the C oracle: centres spread
    `margin_px` past every image edge, so some splats straddle the right and
    bottom edges and some are centred outside.  pin: pixel coordinates for
    splat 0's centre (the projection maps a mean m to (m + 1) size / 2)."""
    rng = np.random.default_rng(seed)
    spread = np.array([1.0 + 2.0 * margin_px / W, 1.0 + 2.0 * margin_px / H])
    means = (rng.uniform(-1.0, 1.0, (n, 2)) * spread).astype(F32)
    if pin is not None:
        means[0] = (2.0 * pin[0] / W - 1.0, 2.0 * pin[1] / H - 1.0)
    L = ((rng.random((n, 3)) + np.array([0.5, 0.0, 0.5])) * chol).astype(F32)
    colors = rng.random((n, 3)).astype(F32)
    opacity = rng.uniform(opac[0], opac[1], (n, 1)).astype(F32)
    tb = O.tile_bounds(H, W)
    xys, depths, radii, conics, nth = O.project_2d_forward(means, L, H, W, tb)
    m, cum = O.cumulative_intersects(nth)
    nt = tb[0] * tb[1]
    if m < 1:
        lists = [np.zeros(0, I32) for _ in range(nt)]
    else:
        _, _, _, gids, bins = O.bin_and_sort(xys, depths, radii, cum, tb, m)
        lists = [gids[bins[t, 0]:bins[t, 1]].astype(I32) for t in range(nt)]
    c = dict(H=H, W=W, seed=seed, xys=xys, conics=conics, colors=colors, opacity=opacity,
             depths=depths, radii=radii, nth=nth, f64=True, claims={})
    c["v_out"] = rng.standard_normal((H, W, 3)).astype(F32)
    c["v_alpha"] = rng.standard_normal((H, W)).astype(F32)
    c["bg"] = np.array([0.1, 0.4, 0.7], F32) if seed % 2 else np.zeros(3, F32)
    return _set_lists(c, lists)


def _set_lists(c, lists):
    """Write the per-tile id lists as gaussian_ids_sorted / tile_bins.  Every id
    is checked to be in range and every bin to lie inside the id array (never
    empty: a list-less frame keeps one unused id), so no kernel can read out
    of bounds on a case."""
    n = c["xys"].shape[0]
    assert len(lists) == _ntiles(c["H"], c["W"])
    lists = [np.asarray(l, I32).reshape(-1) for l in lists]
    counts = np.array([len(l) for l in lists], np.int64)
    ends = np.cumsum(counts)
    gids = np.concatenate(lists + [np.zeros(0, I32)]).astype(I32)
    if gids.size == 0:
        gids = np.zeros(1, I32)
    assert gids.min() >= 0 and gids.max() < n
    bins = np.stack([ends - counts, ends], 1).astype(I32)
    assert bins.min() >= 0 and bins.max() <= gids.size and (bins[:, 0] <= bins[:, 1]).all()
    c["gids"], c["bins"], c["counts"] = gids, bins, counts
    return c


def _tile_centre(c, t):
    tbx = (c["W"] + TILE - 1) // TILE
    ty, tx = divmod(t, tbx)
    x1, y1 = min(c["W"], tx * TILE + TILE), min(c["H"], ty * TILE + TILE)
    return 0.5 * (tx * TILE + x1 - 1), 0.5 * (ty * TILE + y1 - 1)


def _nearest(c, t, n, pool=None, far=False):
    """The n splats of `pool` (default all) nearest to (far: farthest from) tile
    t's centre, in id order (the projection's depth is 0: id order is the sort)."""
    pool = np.arange(c["xys"].shape[0]) if pool is None else np.asarray(pool)
    cx, cy = _tile_centre(c, t)
    d = np.hypot(c["xys"][pool, 0] - cx, c["xys"][pool, 1] - cy)
    order = np.argsort(-d if far else d, kind="stable")[:n]
    return np.sort(pool[order]).astype(I32)


def _shape_case(H, W, seed):
    n = max(16, int(0.075 * (H + 8) * (W + 8)))
    # splat 0 sits inside the bottom right pixel, straddling both edges
    c = _frame(H, W, n, seed, pin=(W - 1 + 0.2, H - 1 - 0.3))
    c.update(id=f"shape-{H}x{W}", path="edge guards pi < img_h, pj + q < img_w; natural lists")
    return c


COUNTS = [257, 0, 1, 7, 8, 9, 24, 25, 63, 64, 65, 88, 89, 128, 129, 0, 257, 24, 25, 1]


def _count_case(faint):
    """50x70 (4 x 5 tiles, both edges partial), per-tile counts COUNTS: the
    forward's 24 | 25 list switch, the 64-entry chunk (64 | 65, remainders 24 |
    25 of 88 | 89), 128 | 129, 257; the backward's groups of 8 (1, 7, 8, 9, 63,
    64, 65, 129); empty tiles next to the fullest.  Faint: no pixel stops.
    Opaque: pixels stop all along the lists."""
    c = (_frame(50, 70, 900, 41, opac=(0.004, 0.03)) if faint else
         _frame(50, 70, 900, 42, opac=(0.6, 0.97), chol=6.0))
    _set_lists(c, [_nearest(c, t, k) for t, k in enumerate(COUNTS)])
    c.update(id="counts-faint" if faint else "counts-opaque",
             path="fwd cnt > kAGroupMin, kAChunk remainders; bwd groups of 8; empty next to full")
    c["claims"]["counts"] = COUNTS
    return c


def _allstop_case(count):
    """32x20 (2 x 2 tiles; tiles 1 and 3 hold 4 columns).  Tile 1: every pixel
    but (15, 19) stops inside the first chunk (rows 0..14: three flat opaque
    row splats each; (15, 16..18): three point splats each), then `count` - 54
    faint entries, the last one the live pixel's own: __all(done) approached, not
    taken.  Tile 3: sixteen rows of three row splats, every pixel stops before
    entry 48, the list goes on to `count`: the exit is taken, and the backward's
    kend cuts every chunk but the first.  Tiles 0, 2: 30 faint entries."""
    H, W, nf = 32, 20, 300
    c = _frame(H, W, nf + 103, 50 + count, opac=(0.004, 0.03))
    xy, con, op = c["xys"], c["conics"], c["opacity"]
    hand = nf  # ids nf.. are rewritten by hand

    def put(x, y, a, cc):
        nonlocal hand
        xy[hand] = (x + 0.03, y + 0.03)  # off the pixel centre: sigma is never ~0
        con[hand] = (a, 0.0, cc)
        op[hand] = 0.97
        hand += 1
        return hand - 1

    t1, t3 = [], []
    for r in range(15):
        t1 += [put(17.5, r, 1e-5, 14.0) for _ in range(3)]
    for col in (16, 17, 18):
        t1 += [put(col, 15, 14.0, 14.0) for _ in range(3)]
    for r in range(16, 32):
        t3 += [put(17.5, r, 1e-5, 14.0) for _ in range(3)]
    # the live pixel's own faint splat closes tile 1's list (the second chunk)
    xy[hand], con[hand], op[hand] = (19.2, 15.3), (0.3, 0.0, 0.3), 0.02
    assert hand == nf + 102 and len(t1) == 54 and len(t3) == 48
    faint = np.arange(nf)
    lists = [_nearest(c, 0, 30, faint),
             np.concatenate([t1, _nearest(c, 1, count - 55, faint), [hand]]),
             _nearest(c, 2, 30, faint), np.concatenate([t3, _nearest(c, 3, count - 48, faint)])]
    _set_lists(c, lists)
    c.update(id=f"allstop-{count}", path="fwd __all(done) exit approached (tile 1) and taken "
             "(tile 3); bwd kend cuts whole chunks")
    c["claims"].update(approached=(1, (15, 19)), taken=3, count=count)
    return c


def ellipse_extent(conic, o):
    """Half-extents (x, y) of the alpha >= 1/255 ellipse, float64."""
    a, b, cc = (float(v) for v in conic)
    s2 = 2.0 * math.log(255.0 * float(o))
    det = a * cc - b * b
    return math.sqrt(s2 * cc / det), math.sqrt(s2 * a / det)


def _blockedge_case():
    """32x35 (2 x 3 tiles); tile 4 (origin 16, 16; 40 entries: grouped lists) holds 16 hand
    placed axis-aligned splats whose alpha >= 1/255 ellipse ends 0.04 px inside
    or outside a 4x4 block's first / last pixel column or row: an entry
    wrongly left out of a block's list (cull.h ellipse_blocks) or of the
    backward's rectangle (rows.h ellipse_rect) changes a non-borderline pixel."""
    H, W = 32, 35
    c = _frame(H, W, 120, 61, opac=(0.2, 0.9))
    rng = np.random.default_rng(62)
    edges, ids = [], []
    g = 100
    for axis in (0, 1):
        for side in (+1, -1):       # +1: the ellipse's far end meets a block's first line
            for inside in (True, False):
                for blk in (1, 2):
                    a, cc, o = rng.uniform(0.3, 0.8), rng.uniform(0.3, 0.8), rng.uniform(0.4, 0.9)
                    con = np.array([a, 0.0, cc], F32)
                    o = F32(o)
                    ext = ellipse_extent(con, o)[axis]
                    line = 16 + 4 * blk + (0 if side > 0 else 3)  # pixel column / row
                    d = 0.04 if inside else -0.04
                    pos = line - side * (ext - d)      # the end is d past the line
                    other = 16 + 4 * blk + 1           # an integer row / column: dy (dx) = 0 there
                    c["xys"][g] = (pos, other) if axis == 0 else (other, pos)
                    c["conics"][g] = con
                    c["opacity"][g] = o
                    edges.append(dict(id=g, axis=axis, side=side, inside=inside, line=line,
                                      other=other))
                    ids.append(g)
                    g += 1
    others = _nearest(c, 4, 24, np.arange(100))
    lists = [np.array([i for i in c["gids"][b0:b1] if i < 100], I32) for b0, b1 in c["bins"]]
    lists[4] = np.sort(np.concatenate([others, np.array(ids, I32)]))
    _set_lists(c, lists)
    c.update(id="blockedge", path="fwd ellipse_blocks / bwd ellipse_rect at +-0.04 px of a line")
    c["claims"]["edges"] = edges
    return c


def _noblend_case():
    """40x36 (3 x 3 tiles): tiles 0 and 4 list the 30 splats farthest from
    them, so no pixel of either blends anything (final_idx 0 everywhere): the
    backward's kend as tile 0 (entry 0 is visited, invalid) and as a later tile
    (kend = 1 < range.x: no chunk at all)."""
    c = _frame(40, 36, 160, 71)
    lists = [c["gids"][b0:b1] for b0, b1 in c["bins"]]
    lists[0] = _nearest(c, 0, 30, far=True)
    lists[4] = _nearest(c, 4, 30, far=True)
    _set_lists(c, lists)
    c.update(id="noblend", path="bwd tile whose pixels blended nothing (tile 0, tile 4)")
    c["claims"]["noblend"] = (0, 4)
    return c


def _nine_case():
    """45x47 (3 x 3 tiles): splat 0, wide, heads every tile's list, so its
    64-byte gradient record is met by atomics from nine tiles."""
    c = _frame(45, 47, 150, 81)
    c["xys"][0] = (23.3, 22.4)
    c["conics"][0] = (0.004, 0.001, 0.005)
    c["opacity"][0] = 0.6
    lists = [np.concatenate([[0], [i for i in c["gids"][b0:b1] if i != 0]]) for b0, b1 in c["bins"]]
    _set_lists(c, lists)
    c.update(id="nine-tiles", path="bwd one record, atomics from nine tiles")
    return c


OPACITIES = [0.0, -0.5, 1.0, 1.5, math.exp(-0.02) / 255, math.exp(-0.005) / 255, 1.01 / 255,
             0.3, 0.7, 0.05]


def _opacity_case():
    """20x37: opacities 0, -0.5, 1, 1.5 and the band around 1/255 on both sides
    of cull.h / rows.h's `lg < -0.01f` cut (e^-0.02 / 255: cut; e^-0.005 / 255:
    kept by the cut, alpha < 1/255 everywhere; 1.01 / 255: alpha >= 1/255 only
    within ~0.2 px of the centre, which sits 0.02 px off a pixel centre)."""
    c = _frame(20, 37, 130, 91)
    n = c["xys"].shape[0]
    k = np.arange(n) % len(OPACITIES)
    c["opacity"][:, 0] = np.array(OPACITIES, F32)[k]
    near = k == 6
    c["xys"][near] = np.round(c["xys"][near]) + F32(0.02)
    c.update(id="opacities", path="opacity 0, < 0, 1, > 1, the 1/255 band of the culls' cut")
    return c


def _clamp_case():
    """17x17: opacity 1 and 0.995 splats 0.03 px off pixel centres, so blended
    alphas lie in (0.99, 0.999]: the forward's 0.999 and the backward's 0.99
    clamps.  Gradients go against the recursion only."""
    c = _frame(17, 17, 40, 101)
    n = c["xys"].shape[0]
    c["opacity"][:, 0] = np.where(np.arange(n) % 2 == 0, 1.0, 0.995).astype(F32)
    c["xys"][:] = np.round(c["xys"]) + F32(0.03)
    c.update(id="clamp-99", path="alpha in (0.99, 0.999]: fwd clamp 0.999, bwd clamp 0.99")
    return c


def _caller_case(kind):
    """20x20, natural lists plus splat 0 rewritten and listed in every tile."""
    c = _frame(20, 20, 30, {"nonpd": 111, "needle": 113, "nancolor": 115}[kind], opac=(0.2, 0.9))
    c["xys"][0] = (10.3, 9.6)
    if kind == "nonpd":
        c["conics"][0] = (0.05, 0.2, 0.05)       # det < 0: sigma < 0 where dx dy < 0
    elif kind == "needle":
        c["conics"][0] = (136777.0, -90809.8, 60291.0)  # a c > 8192 det: cull_conditioned's escape
        c["opacity"][0] = 1.0
    else:
        c["colors"][0, 1] = np.nan
    lists = [np.concatenate([[0], [i for i in c["gids"][b0:b1] if i != 0]]) for b0, b1 in c["bins"]]
    _set_lists(c, lists)
    c.update(id=f"caller-{kind}", f64=False, path="op-level caller geometry, against the C oracle")
    return c


def _build_cases():
    cases = [_shape_case(H, W, 11 + i) for i, (H, W) in enumerate(
        [(1, 1), (1, 37), (37, 1), (5, 3), (15, 17), (17, 15), (33, 18), (20, 70), (37, 45)])]
    cases += [_count_case(True), _count_case(False)]
    cases += [_allstop_case(n) for n in (65, 89, 129, 257)]
    cases += [_blockedge_case(), _noblend_case(), _nine_case(), _opacity_case(), _clamp_case()]
    cases += [_caller_case(k) for k in ("nonpd", "needle", "nancolor")]
    return cases


CASES = _build_cases()
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)
F64_IDS = [c["id"] for c in CASES if c["f64"]]
CALLER_IDS = [c["id"] for c in CASES if not c["f64"]]
GLUE_ID = "shape-37x45"


# ---------------------------------------------------------------- references
def _tiles(c):
    """(tile, rows ii, columns jj, r0, r1) of every tile: its in-image pixels."""
    H, W = c["H"], c["W"]
    tbx = (W + TILE - 1) // TILE
    for t, (r0, r1) in enumerate(c["bins"]):
        ty, tx = divmod(t, tbx)
        ii, jj = np.mgrid[ty * TILE:min(H, ty * TILE + TILE), tx * TILE:min(W, tx * TILE + TILE)]
        yield t, ii.ravel(), jj.ravel(), int(r0), int(r1)


def _geo64(c):
    return (c["xys"].astype(F64), c["conics"].astype(F64), c["colors"].astype(F64),
            c["opacity"].astype(F64).reshape(-1), c["bg"].astype(F64))


def _sigma(xy, con, g, ii, jj):
    dx, dy = xy[g, 0] - jj, xy[g, 1] - ii
    a, b, cc = con[g]
    return dx, dy, 0.5 * (a * dx * dx + cc * dy * dy) + b * dx * dy


def alpha_forward64(c):
    """forward.cu:252-374 in float64, per tile, entries in list order: skip an
    entry if sigma < 0 or min(0.999, o e^-sigma) < 1/255; stop, without
    blending it, at the entry with T (1 - alpha) <= 1e-4; out = acc + T bg;
    final_idx = the last blended list position, 0 if none.  Also: `borderline`
    (a decision of a still-live pixel within a relative 1e-4 of its threshold,
    or |sigma| < 1e-6 -- four orders above float32 exp error, so float32 can
    only decide differently inside it), `hi99` (a blended raw alpha >
    0.99 (1 - 1e-4)), `stopped` / `stop_pos` (the list position, within the
    tile, of the stopping entry) and per tile the blend mask [pixels, entries]."""
    H, W = c["H"], c["W"]
    xy, con, col, op, bg = _geo64(c)
    out = np.zeros((H, W, 3))
    Tf = np.ones((H, W))
    idx = np.zeros((H, W), I32)
    border = np.zeros((H, W), bool)
    hi99 = np.zeros((H, W), bool)
    stopped = np.zeros((H, W), bool)
    stop_pos = np.full((H, W), -1, np.int64)
    blend = []
    with np.errstate(over="ignore", invalid="ignore"):
        for t, ii, jj, r0, r1 in _tiles(c):
            P = ii.size
            T, acc = np.ones(P), np.zeros((P, 3))
            last, done = np.zeros(P, np.int64), np.zeros(P, bool)
            bd, h9, sp = np.zeros(P, bool), np.zeros(P, bool), np.full(P, -1, np.int64)
            B = np.zeros((P, r1 - r0), bool)
            for k in range(r0, r1):
                g = c["gids"][k]
                _, _, s = _sigma(xy, con, g, ii, jj)
                raw = op[g] * np.exp(-s)
                al = np.minimum(0.999, raw)
                live = ~done
                bd |= live & (np.abs(s) < SIGMA_MARGIN)
                bd |= live & (np.abs(al * 255.0 - 1.0) < MARGIN)
                valid = live & ~(s < 0) & ~(al < ALPHA_MIN)
                nT = T * (1.0 - al)
                bd |= valid & (np.abs(nT / T_STOP - 1.0) < MARGIN)
                stop = valid & (nT <= T_STOP)
                upd = valid & ~stop
                sp[stop] = k - r0
                done |= stop
                acc[upd] += (al * T)[upd, None] * col[g]
                T = np.where(upd, nT, T)
                last[upd] = k
                h9 |= upd & (raw > 0.99 * (1.0 - MARGIN))
                B[:, k - r0] = upd
            out[ii, jj] = acc + T[:, None] * bg
            Tf[ii, jj], idx[ii, jj], border[ii, jj], hi99[ii, jj] = T, last, bd, h9
            stopped[ii, jj], stop_pos[ii, jj] = done, sp
            blend.append(B)
    return dict(out=out, T=Tf, idx=idx, borderline=border, hi99=hi99, stopped=stopped,
                stop_pos=stop_pos, blend=blend)


def upstream(c, borderline, which="both"):
    """(v_out, v_out_alpha) float32 of the case, zeroed on the borderline pixels
    (a decision flipped there must not leak into a splat's sum); `which`:
    'both', 'out' (v_out_alpha = 0) or 'alpha' (v_out = 0)."""
    vo, va = c["v_out"].copy(), c["v_alpha"].copy()
    vo[borderline] = 0
    va[borderline] = 0
    if which == "out":
        va[:] = 0
    if which == "alpha":
        vo[:] = 0
    return vo, va


def lowered_idx(c, idx, share=0.1, seed=17):
    """final_idx lowered on a random `share` of the pixels to a position
    anywhere in the pixel's tile list at or below its own (a caller's
    final_idx, not the one the forward implies)."""
    rng = np.random.default_rng(seed)
    out = np.array(idx, I32)
    for t, ii, jj, r0, r1 in _tiles(c):
        if r1 <= r0:
            continue
        cur = out[ii, jj]
        pick = (rng.random(ii.size) < share) & (cur > r0)
        low = r0 + np.floor(rng.random(ii.size) * (cur - r0)).astype(I32)
        out[ii, jj] = np.where(pick, low, cur)
    return out


def alpha_backward64_recursion(c, final_T, final_idx, v_out, v_alpha):
    """backward.cu:225-290 in float64: per pixel, back to front over the
    entries k <= final_idx that are valid under the BACKWARD's clamp (alpha =
    min(0.99, o e^-sigma), skip if sigma < 0 or alpha < 1/255), T rolled back
    by 1 / (1 - alpha), the colour buffer, v_alpha, v_sigma = -o e^-sigma
    v_alpha; v_conic's cross term is the reference's 1/2 v_sigma dx dy."""
    xy, con, col, op, bg = _geo64(c)
    n = xy.shape[0]
    g_xy, g_con, g_col, g_op = np.zeros((n, 2)), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 1))
    final_T, v_out, v_alpha = (np.asarray(a, F64) for a in (final_T, v_out, v_alpha))
    with np.errstate(over="ignore", invalid="ignore"):
        for t, ii, jj, r0, r1 in _tiles(c):
            Tfin = final_T[ii, jj]
            T, buf = Tfin.copy(), np.zeros((ii.size, 3))
            bf, vo, va = np.asarray(final_idx)[ii, jj], v_out[ii, jj], v_alpha[ii, jj]
            for k in range(r1 - 1, r0 - 1, -1):
                g = c["gids"][k]
                dx, dy, s = _sigma(xy, con, g, ii, jj)
                vis = np.exp(-s)
                al = np.minimum(0.99, op[g] * vis)
                m = (k <= bf) & ~(s < 0) & ~(al < ALPHA_MIN)
                if not m.any():
                    continue
                dx, dy, vis, al = dx[m], dy[m], vis[m], al[m]
                ra = 1.0 / (1.0 - al)
                Tn = T[m] * ra
                fac = al * Tn
                tfra = Tfin[m] * ra
                v_al = ((col[g] * Tn[:, None] - buf[m] * ra[:, None]) * vo[m]).sum(1)
                v_al += tfra * va[m] - tfra * (vo[m] @ bg)
                buf[m] += fac[:, None] * col[g]
                T[m] = Tn
                v_s = -op[g] * vis * v_al
                a, b, cc = con[g]
                g_col[g] += (fac[:, None] * vo[m]).sum(0)
                g_con[g] += [(0.5 * v_s * dx * dx).sum(), (0.5 * v_s * dx * dy).sum(),
                             (0.5 * v_s * dy * dy).sum()]
                g_xy[g] += [(v_s * (a * dx + b * dy)).sum(), (v_s * (b * dx + cc * dy)).sum()]
                g_op[g] += (vis * v_al).sum()
    return dict(v_xy=g_xy, v_conic=g_con, v_colors=g_col, v_opacity=g_op)


def alpha_backward64_autograd(c, fwd, v_out, v_alpha):
    """Autograd of the float64 forward with every decision fixed to `fwd`'s
    blend masks (the clamp is inactive: valid only where fwd['hi99'] is empty
    and final_idx is the forward's own), loss = sum out v_out + sum (1 - T)
    v_alpha; the v_conic cross term halved (the reference's quirk)."""
    assert not fwd["hi99"].any()
    xy, con, col, op = (torch.tensor(a, dtype=torch.float64, requires_grad=True)
                        for a in _geo64(c)[:4])
    bg = torch.tensor(c["bg"], dtype=torch.float64)
    vo_all, va_all = torch.tensor(v_out, dtype=torch.float64), torch.tensor(v_alpha, dtype=torch.float64)
    loss = torch.zeros((), dtype=torch.float64)
    for (t, ii, jj, r0, r1), B in zip(_tiles(c), fwd["blend"]):
        if r1 <= r0 or not B.any():
            continue
        g = torch.tensor(c["gids"][r0:r1].astype(np.int64))
        Bt = torch.tensor(B)
        dx = xy[g, 0][None, :] - torch.tensor(jj, dtype=torch.float64)[:, None]
        dy = xy[g, 1][None, :] - torch.tensor(ii, dtype=torch.float64)[:, None]
        s = 0.5 * (con[g, 0] * dx * dx + con[g, 2] * dy * dy) + con[g, 1] * dx * dy
        al = torch.where(Bt, op[g] * torch.exp(-torch.where(Bt, s, torch.zeros_like(s))),
                         torch.zeros_like(s))
        Tinc = torch.cumprod(1.0 - al, dim=1)
        Texc = torch.cat([torch.ones_like(Tinc[:, :1]), Tinc[:, :-1]], 1)
        Tfin = Tinc[:, -1]
        out = (al * Texc) @ col[g] + Tfin[:, None] * bg
        loss = loss + (out * vo_all[ii, jj]).sum() + ((1.0 - Tfin) * va_all[ii, jj]).sum()
    if loss.requires_grad:
        loss.backward()
    z = lambda p: np.zeros(tuple(p.shape)) if p.grad is None else p.grad.numpy().copy()
    g_con = z(con)
    g_con[:, 1] *= 0.5
    return dict(v_xy=z(xy), v_conic=g_con, v_colors=z(col), v_opacity=z(op).reshape(-1, 1))


_ref_cache = {}


def reference(cid):
    """The float64 forward of a case, its upstream (borderline zeroed) and the
    recursion gradients for it, computed once per process and never written."""
    if cid not in _ref_cache:
        c = BY_ID[cid]
        fwd = alpha_forward64(c)
        vo, va = upstream(c, fwd["borderline"])
        rec = alpha_backward64_recursion(c, fwd["T"], fwd["idx"], vo, va)
        _ref_cache[cid] = dict(fwd=fwd, v_out=vo, v_alpha=va, rec=rec)
    return _ref_cache[cid]


VARIANT_IDS = [(cid, v) for cid in (GLUE_ID, "counts-opaque") for v in ("out", "alpha", "lowered")]


def variant(cid, kind):
    """Backward-only variants of a case: v_out alone ('out'), v_out_alpha alone
    ('alpha'), or a caller-lowered final_idx on 10 % of the pixels ('lowered':
    only the recursion is a reference then).  Returns (v_out, v_out_alpha,
    final_idx, recursion gradients), the forward being the case's own."""
    key = (cid, kind)
    if key not in _ref_cache:
        c, fwd = BY_ID[cid], reference(cid)["fwd"]
        vo, va = upstream(c, fwd["borderline"], "both" if kind == "lowered" else kind)
        fi = lowered_idx(c, fwd["idx"]) if kind == "lowered" else fwd["idx"]
        _ref_cache[key] = (vo, va, fi, alpha_backward64_recursion(c, fwd["T"], fi, vo, va))
    return _ref_cache[key]


# ---------------------------------------------------------------- error measures
def edge_splats(c):
    """Splats centred within EDGE_PX of the right or bottom image edge (or
    past it) that some tile lists."""
    xy = c["xys"]
    listed = np.zeros(xy.shape[0], bool)
    for r0, r1 in c["bins"]:
        listed[c["gids"][r0:r1]] = True
    return listed & ((xy[:, 0] >= c["W"] - 1 - EDGE_PX) | (xy[:, 1] >= c["H"] - 1 - EDGE_PX))


def rel_error(got, ref):
    """max |got - ref| relative to ref's largest element; where ref is all zero
    got must be zero too (0, else inf)."""
    got, ref = np.asarray(got, F64).reshape(np.shape(ref)), np.asarray(ref, F64)
    if ref.size == 0:
        return 0.0
    d, top = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    if top == 0.0:
        return 0.0 if d == 0.0 else math.inf
    return d / top


def assert_within_bar(got, ref, name):
    """got against a float32 reference (a golden file, the C oracle) under
    BARS[name]: image and T absolute, a gradient relative to ref's largest
    element."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64).reshape(np.shape(got))
    err = float(np.abs(got - ref).max()) if name in ("image", "T") else rel_error(got, ref)
    assert err <= BARS[name], (name, err, BARS[name])


def grad_errors(c, got, ref):
    """name -> (whole, edge): each gradient's error over the whole tensor
    relative to its largest element, and over the edge splats relative to that
    subset's largest (a lost edge column must not hide under an interior
    maximum)."""
    e = edge_splats(c)
    res = {}
    for name, g in zip(GRADS, got):
        g = np.asarray(g, F64).reshape(ref[name].shape)
        res[name] = (rel_error(g, ref[name]), rel_error(g[e], ref[name][e]))
    return res


def oracle_run(c, v_out, v_alpha, final_idx=None):
    """The C oracle (float32) on a case: forward, then backward on its own
    final_Ts and final_idx (or the caller's `final_idx`)."""
    H, W = c["H"], c["W"]
    tb = O.tile_bounds(H, W)
    args = (c["gids"], c["bins"], c["xys"], c["conics"], c["colors"], c["opacity"], c["bg"])
    out, Ts, idx = O.raster_forward(tb, H, W, *args)
    g = O.raster_backward(tb, H, W, *args, Ts, idx if final_idx is None else final_idx, v_out,
                          v_alpha)
    return out, Ts, idx, g
