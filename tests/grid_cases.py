"""Tile grids past anything the scripted cases reach, shared by
test_grid_cases_cpu.py (premises, no GPU), test_tile_grids.py (the HIP kernels)
and tests/analysis/sum_bars.py.  Nothing here imports the code under test.

Binning grids (BIN_GRIDS, given as (tbx, tby); no image): ~3000 splats with
integer radii and centres on multiples of 1/64 px, so cx / 16, +- r / 16 and + 1
are exact in float32 and float64 alike and no tile box is borderline.  The
reference (bin_reference) is integer numpy in units of 1/64 px: boxes,
num_tiles_hit, the emission order of the map kernel, the (tile, id)
lexicographic order, tile_bins (uncapped and capped at 256) and M.  The grids
sit on the tile counts at which the binning changes behaviour: the radix sort's
bits_for(tiles) = 0, 1, 8, 9, 16, 17 and the scan's chunks of SCAN_CHUNK = 8192
tiles (exactly one, one tile more, a second and third trip, nine trips).

Rendered grids (RENDER_GRIDS): sparse frames of 525, 8385 and 16512 tiles built
with sum_cases' helpers and passed through sum_cases.fused_case's nudging loop
(registered there as fused cases "grid-R2", "grid-R1", "grid-R3" and their L1
variants), so the float64 references, the margins and the error measures are
sum_cases' own."""
import numpy as np

import sum_cases as S

F32, F64, I32, I64 = np.float32, np.float64, np.int32, np.int64
SCAN_CHUNK = 8192    # binning.h scan_tile_counts<1024, 8>: tiles per trip
LOSS_TRIP = 8192     # train.hip publish_loss<256>, kLossBatch 16: 4096 tile pairs per trip
TILE_CAP = 256
SUB = 64             # centre units per pixel
UNIT = 16 * SUB      # centre units per tile

BIN_GRIDS = [(1, 1), (2, 1), (16, 16), (257, 1), (1, 257), (128, 64), (2731, 3), (129, 65),
             (129, 128), (256, 256), (257, 256)]
BIN_IDS = [f"{x}x{y}" for x, y in BIN_GRIDS]
SORT_BITS = {1: 0, 2: 1, 256: 8, 257: 9, 8192: 13, 8193: 14, 8385: 14, 16512: 15, 65536: 16, 65792: 17}
_bin_cache = {}


def bits_for(count):
    b = 0
    while (1 << b) < count:
        b += 1
    return b


def joins(ntiles):
    """The first tile of every scan chunk after the first."""
    return list(range(SCAN_CHUNK, ntiles, SCAN_CHUNK))


def placements(tbx, tby):
    """tile -> one-tile splats placed there on purpose: tile 0, the last tile,
    both tiles of every chunk join (different counts), a tile past 256 entries
    in the first chunk, and after the first join one above 64 and one above
    256 (one tile for both where the grid has a single tile there)."""
    nt = tbx * tby
    want = {0: 3}
    if nt > 1:
        want[nt - 1] = 7
    if nt > 2:
        want[min(100, nt // 3)] = 300
    for k, j in enumerate(joins(nt)):
        want[j - 1] = 5 + k
        want[j] = 11 + 2 * k
    if nt >= SCAN_CHUNK + 8:
        want[SCAN_CHUNK + 3] = 70
        want[SCAN_CHUNK + 6] = 300
    elif nt > SCAN_CHUNK:
        want[SCAN_CHUNK] = 300
    return want


def _one_tile(rng, tiles, tbx):
    """One-tile splats (radius 1..5, the whole disc's box inside the tile) in
    the given tiles: (cx, cy, r) in centre units / pixels."""
    tiles = np.asarray(tiles, I64)
    r = rng.integers(1, 6, tiles.size)
    ox = rng.integers(SUB * r + 1, UNIT - SUB * r)
    oy = rng.integers(SUB * r + 1, UNIT - SUB * r)
    return np.stack([(tiles % tbx) * UNIT + ox, (tiles // tbx) * UNIT + oy, r], 1)


def bin_grid(tbx, tby):
    """The splats of a binning grid: xys float32 [n, 2], radii int32 [n], depths
    zeros, and the same in integers (`cxy` in 1/64 px)."""
    key = (tbx, tby)
    if key in _bin_cache:
        return _bin_cache[key]
    rng = np.random.default_rng(9000 + 7 * tbx + tby)
    nt, X, Y = tbx * tby, tbx * UNIT, tby * UNIT
    rows = []
    # radius 0 anywhere: listed nowhere
    rows.append(np.stack([rng.integers(0, X, 200), rng.integers(0, Y, 200), np.zeros(200, I64)], 1))
    # one tile each, and 3 x 3 (radius 16 from anywhere inside a tile)
    rows.append(_one_tile(rng, rng.integers(0, nt, 1300), tbx))
    rows.append(np.stack([rng.integers(0, X, 500), rng.integers(0, Y, 500), np.full(500, 16, I64)], 1))
    # centres off the grid on every side, up to 40 px out: some reach back in
    off = rng.integers(1, 40 * SUB, 240)
    along_x, along_y = rng.integers(-20 * SUB, X + 20 * SUB, 240), rng.integers(-20 * SUB, Y + 20 * SUB, 240)
    side = np.arange(240) % 4
    cx = np.where(side == 0, -off, np.where(side == 1, X - 1 + off, along_x))
    cy = np.where(side == 2, -off, np.where(side == 3, Y - 1 + off, along_y))
    rows.append(np.stack([cx, cy, rng.choice([0, 4, 16, 48], 240)], 1))
    # two that span the grid's longer side (a whole tile row or column of a thin grid)
    span = 8 * max(tbx, tby) + 8
    rows.append(np.array([[X // 2 + 5, Y // 2 - 3, span], [X // 2 - 130, Y // 2 + 77, span]], I64))
    want = placements(tbx, tby)
    for t, k in sorted(want.items()):
        rows.append(_one_tile(rng, np.full(k, t), tbx))
    s = np.concatenate(rows).astype(I64)
    s = s[rng.permutation(s.shape[0])]
    xys = (s[:, :2].astype(F64) / SUB).astype(F32)
    assert (xys.astype(F64) * SUB == s[:, :2]).all()  # multiples of 1/64 px are exact in float32
    g = dict(tbx=tbx, tby=tby, ntiles=nt, n=s.shape[0], cxy=s[:, :2].copy(), xys=xys,
             radii=s[:, 2].astype(I32), depths=np.zeros(s.shape[0], F32), placed=want)
    g["ref"] = bin_reference(g)
    _bin_cache[key] = g
    return g


def bin_reference(g):
    """Integer numpy: helpers.cuh's tile box [x0, x1) x [y0, y1) (truncation
    toward zero and the clamp to [0, tb] agree with floor division once
    clamped), num_tiles_hit and its inclusive sum, the (tile, id) pairs in the
    map kernel's emission order (splat order, row-major over the box), their
    lexicographic order, per-tile counts, tile_bins and M."""
    tbx, tby, nt = g["tbx"], g["tby"], g["ntiles"]
    c, r = g["cxy"], g["radii"].astype(I64)
    x0 = np.clip((c[:, 0] - SUB * r) // UNIT, 0, tbx)
    x1 = np.clip((c[:, 0] + SUB * r + UNIT) // UNIT, 0, tbx)
    y0 = np.clip((c[:, 1] - SUB * r) // UNIT, 0, tby)
    y1 = np.clip((c[:, 1] + SUB * r + UNIT) // UNIT, 0, tby)
    w, h = np.where(r > 0, x1 - x0, 0), np.where(r > 0, y1 - y0, 0)
    w, h = np.maximum(w, 0), np.maximum(h, 0)
    nth = w * h
    cum = np.cumsum(nth)
    M = int(cum[-1])
    assert M < 2 ** 31
    ids = np.repeat(np.arange(g["n"], dtype=I64), nth)
    k = np.arange(M, dtype=I64) - np.repeat(cum - nth, nth)
    wr = np.repeat(np.maximum(w, 1), nth)
    tiles = (np.repeat(y0, nth) + k // wr) * tbx + np.repeat(x0, nth) + k % wr
    order = np.lexsort((ids, tiles))
    counts = np.bincount(tiles, minlength=nt).astype(I64)

    def bins_of(cnt):
        end = np.cumsum(cnt)
        b = np.stack([end - cnt, end], 1)
        b[cnt == 0] = 0
        return b.astype(I32)

    capped = np.minimum(counts, TILE_CAP)
    bins = bins_of(counts)
    gids = ids[order].astype(I32)
    gids_capped = np.concatenate([gids[s:s + k] for (s, _), k in zip(bins, capped)] + [np.zeros(0, I32)])
    return dict(box=np.stack([x0, x1, y0, y1], 1), nth=nth.astype(I32), cum=cum.astype(I32), M=M,
                map_tiles=tiles, map_ids=ids.astype(I32), isect=tiles << 32,
                isect_sorted=tiles[order] << 32, gids=gids, counts=counts, bins=bins,
                bins_capped=bins_of(capped), gids_capped=gids_capped.astype(I32),
                M_capped=int(capped.sum()))


# ---------------------------------------------------------------- rendered grids
RENDER_GRIDS = {"R2": (336, 400), "R1": (1031, 2059), "R3": (2040, 2059)}  # (H, W)
K_CYCLE = (1, 9, 65, 130)
OCCUPIED = 40
N_LARGE = 12
GRID_IDS = ["grid-R2", "grid-R2-L1", "grid-R1", "grid-R1-L1", "grid-R3"]
STEP_IDS = GRID_IDS[:4]          # the fused step runs on R2 and R1; R3 is forward only
FORWARD_IDS = ["grid-R2", "grid-R1", "grid-R3"]
_op_cache = {}


def grid_dims(name):
    H, W = RENDER_GRIDS[name]
    return H, W, (W + 15) // 16, (H + 15) // 16


def required_tiles(name):
    """The occupied tiles a rendered grid must have: tile 0, the last tile, the
    last tile of the last full tile row, 8190..8193 (both sides of the scan
    chunk and of the loss trip), the first and last blocks of the xcd_runs<16>
    tail (tiles at or past (ntiles / 128) * 128) and both sides of the
    xcd_remap tail (ntiles / 8) * 8."""
    H, W, tbx, tby = grid_dims(name)
    nt = tbx * tby
    full_rows = tby if H % 16 == 0 else tby - 1
    tail = (nt // 128) * 128
    t = [0, nt - 1, full_rows * tbx - 1, tail, tail + 1, tail + 2, (tail + nt) // 2, nt - 2,
         (nt // 8) * 8 - 1, (nt // 8) * 8]
    t += [8190, 8191, 8192, 8193]
    return sorted({x for x in t if 0 <= x < nt})


def _build_grid(cid):
    name = cid.split("-")[1]
    H, W, tbx, tby = grid_dims(name)
    nt = tbx * tby
    rng = np.random.default_rng(300 + nt)
    must = required_tiles(name)
    rest = rng.choice(np.setdiff1d(np.arange(nt), must), OCCUPIED - len(must), replace=False)
    tiles = np.sort(np.concatenate([must, rest]))
    Ls, cs, cols, tile_of, counts = [], [], [], [], {}
    for i, t in enumerate(tiles):
        k = K_CYCLE[i % 4]
        L = S._small_L(rng, k)
        Ls.append(L)
        cs.append(S._one_tile_centres(rng, int(t), L, H, W))
        cols.append(rng.uniform(-0.3, 1.0, (k, 3)) * 20.0 / k)
        tile_of += [int(t)] * k
        counts[int(t)] = k
    # larger splats across tile joins and the image edges: a third anywhere, a
    # third centred in the last pixels of the right edge, a third of the bottom
    L = S._small_L(rng, N_LARGE) * rng.uniform(4.0, 8.0, (N_LARGE, 1)).astype(F32)
    c = np.stack([rng.uniform(1.0, W - 1.0, N_LARGE), rng.uniform(1.0, H - 1.0, N_LARGE)], 1)
    c[4:8, 0] = W - rng.uniform(0.5, 6.0, 4)
    c[8:12, 1] = H - rng.uniform(0.5, 6.0, 4)
    Ls.append(L)
    cs.append(c)
    cols.append(rng.uniform(-0.3, 1.0, (N_LARGE, 3)) * 0.02)
    tile_of += [-1] * N_LARGE
    L, centres, col = np.concatenate(Ls), np.concatenate(cs), np.concatenate(cols)
    # The box margin is relative (sum_cases.MARGIN of the tile coordinate): at tile column
    # 128 it is 0.2 px, twice the clearance _one_tile_centres leaves.  Redraw the centres
    # that start inside it (the projection alone, no raster), so that fused_case's loop --
    # a full float64 render per round -- has the cut and the clamp left to settle.
    tiles_of = np.asarray(tile_of)
    for _ in range(60):
        pr = S.project_np(np.tanh(S._raw_xyz(centres, H, W).astype(F64)), L.astype(F64), H, W)
        bad = np.flatnonzero(pr["m_box"] < 3.0 * S.MARGIN)
        if not bad.size:
            break
        for i in bad:
            if tiles_of[i] >= 0:
                centres[i] = S._one_tile_centres(rng, int(tiles_of[i]), L[i:i + 1], H, W)[0]
            else:
                centres[i] += rng.uniform(-0.45, 0.45, 2)
    perm = rng.permutation(L.shape[0])
    p = S._params(H, W, S._raw_xyz(centres[perm], H, W), L[perm], col[perm].astype(F32), 400 + nt,
                  loss="L1" if cid.endswith("L1") else "L2")
    p["claims"].update(tile_of=np.asarray(tile_of)[perm], placed=counts, grid=name)
    return p


for _cid in GRID_IDS:
    S.register_fused(_cid, _build_grid)


def grid_case(cid):
    """(p, r) of sum_cases.fused_case: the parameters after the nudging loop
    and the float64 reference."""
    return S.fused_case(cid)


def occupied(r):
    return np.flatnonzero(r["c"]["counts"] > 0)


def tile_mask(H, W, tiles):
    """[H, W] bool: the pixels of the given tiles."""
    tbx, tby = (W + 15) // 16, (H + 15) // 16
    m = np.zeros(tbx * tby, bool)
    m[np.asarray(tiles, I64)] = True
    return np.repeat(np.repeat(m.reshape(tby, tbx), 16, 0), 16, 1)[:H, :W]


def op_case(cid):
    """The op-level view of a rendered grid: the float32 projection (numpy, the
    formulas of sum_cases.project_np in float32) of the case's parameters as
    the operator's inputs, the float64 reference's lists, and the float64
    forward of exactly these inputs."""
    if cid not in _op_cache:
        p, r = grid_case(cid)
        H, W = p["H"], p["W"]
        means, L, colors = S.activated32(p)
        pr = S.project_np(means, L, H, W, F32)
        box = pr["box"]
        c = dict(H=H, W=W, xys=pr["xy"].astype(F32), conics=pr["conic"].astype(F32), colors=colors,
                 opacity=np.ones((means.shape[0], 1), F32), radii=pr["radius"].astype(I32),
                 nth=((box[:, 1] - box[:, 0]) * (box[:, 3] - box[:, 2])).astype(I32), box=box,
                 gids=r["c"]["gids"], bins=r["c"]["bins"], counts=r["c"]["counts"])
        c["fwd"] = S.sum_forward64(c)
        _op_cache[cid] = c
    return _op_cache[cid]


# ---------------------------------------------------------------- losses: sensitivity and restatement
def tile_sums(img, gt, dt=F64, seq=False):
    """Per tile (row-major) the sums of d^2 and |d| over its in-image pixels and
    three channels, in `dt`; seq: strictly sequential in that format (channel,
    row, column order)."""
    C, H, W = img.shape
    tbx, tby = (W + 15) // 16, (H + 15) // 16
    d = (img.astype(dt) - gt.astype(dt).reshape(img.shape))
    pad = np.zeros((C, tby * 16, tbx * 16), dt)
    pad[:, :H, :W] = d
    t = pad.reshape(C, tby, 16, tbx, 16).transpose(1, 3, 0, 2, 4).reshape(tby * tbx, C * 256)
    if seq:  # padding adds exact zeros: the running sums are those of the in-image pixels
        return (np.cumsum(t * t, 1, dtype=dt)[:, -1], np.cumsum(np.abs(t), 1, dtype=dt)[:, -1])
    return (t * t).sum(1), np.abs(t).sum(1)


def pair_sums(s):
    """Tile pairs (2k, 2k + 1) as publish_loss reads them; an odd last tile on
    its own."""
    s = np.asarray(s, F64)
    n = s.size // 2
    pairs = s[:2 * n].reshape(n, 2).sum(1)
    return np.concatenate([pairs, s[2 * n:]])


def loss_sensitivity(cid):
    """(mse, l1): the smallest share of either loss that a single tile pair
    (or the odd last tile) contributes, from the float64 reference alone."""
    p, r = grid_case(cid)
    s2, s1 = tile_sums(r["render"], p["gt"])
    return float(pair_sums(s2).min() / s2.sum()), float(pair_sums(s1).min() / s1.sum())


def tiled_losses32(render32, gt):
    """The summation publish_loss documents, restated: float32 sequential sums
    inside a tile, float64 across tiles."""
    s2, s1 = tile_sums(np.asarray(render32, F32), np.asarray(gt, F32), F32, True)
    numel = float(np.asarray(render32).size)
    return float(s2.astype(F64).sum() / numel), float(s1.astype(F64).sum() / numel)


def float32_fused(p):
    """sum_cases.float32_fused with the losses of tiled_losses32: a sequential
    float32 sum over millions of pixels would only loosen the loss bar."""
    r = S.chain_np(p, F32, True)
    return r["render"], tiled_losses32(r["render"], p["gt"]), r["grads"]


def grid_errors(cid, render, losses, grads):
    """sum_cases.fused_errors with the per-tile gradient measure switched on."""
    p, r = grid_case(cid)
    ref_l = np.asarray(r["losses"], F64)
    dl = np.abs(np.asarray(losses, F64)[:2] - ref_l)
    e = dict(render=float(np.abs(np.asarray(render, F64).reshape(r["render"].shape) - r["render"]).max()),
             loss_abs=float(dl.max()), loss_rel=float((dl / ref_l).max()))
    grads = np.asarray(grads, F64)
    for name, sl in S.PARAM_GRADS:
        e[name] = S.grad_errors(r["c"], grads[:, sl], r["grads"][:, sl], per_tile=True)
    return e
