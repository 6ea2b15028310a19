"""The pooled backward rounds of the training tile kernel (train.hip,
train_tile_band_kernel step 4): the rectangle rows of a
tile's entries over both bands are one item table per chunk, laid out in eight
length classes (widths 15-16, ..., 1-2; entries without items last), its
rounds of 64 items dealt to the two waves as a snake (0, 1, 1, 0, ...), runs of
up to 16 lanes summed by the long form of the DPP segmented scan.

Every case gives its splats explicitly: small ones drawn from a pool and chosen
by the rows of their alpha >= 1/255 rectangle (sum_cases.rect64), and sized
ones (`_sized`: a rectangle of a given width and height at a given place).
`_layout` restates the kernel's table and `test_case_is_what_it_claims` asserts
each case's claim on its float64 reference after the margin loop, on the CPU,
before anything is compared.

Held to, per case (sum_cases.fused_case references, sum_cases.BARS):

* the gradients-only step and a train_iter step with the Adan update (lr 0),
  under the deterministic backward, against float64; the clamped render
  bitwise equal to the frame render's;
* bitwise, three train_iter steps with carried bins against re-projected ones;
* bitwise, two deterministic runs; the deterministic against the plain
  backward on every splat that touches one tile (one flush either way);
* bitwise, both losses against LOSS_BITS, recorded from the parent build (per
  band tables, commit e5bebea): the forward and the loss are untouched.
"""
import math
import os
import re

import numpy as np
import pytest
import torch

import sum_cases as S
import test_sum_edges as E

pytestmark = pytest.mark.gpu

F32 = np.float32
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gsvc_amd", "csrc", "train.hip")
with open(SRC) as _f:
    KBRUN = int(re.search(r"constexpr int kBRun = (\d+);", _f.read()).group(1))  # rows wider than this split in two
K_RECT = math.sqrt(2.0 * (math.log(255.0) * 1.001 + 0.01)) * 1.001  # rows.h ellipse_rect: extent = K sigma + 0.01

# case -> (H, W, loss)
CASES = {
    "items64": (16, 16, "L2"),      # the tile's items: one round, wave 1 idle
    "items65": (16, 16, "L2"),      # two rounds, the second of one item
    "items65-L1": (16, 16, "L1"),
    "items128": (16, 16, "L2"),     # two full rounds
    "items129": (16, 16, "L2"),     # an odd third round (wave 1's second, by the snake)
    "tall-row": (16, 16, "L2"),     # a 16-item run filling one 16-lane DPP row
    "tall-cross": (16, 16, "L2"),   # ... crossing a DPP row inside a round
    "tall-waves": (16, 16, "L2"),   # ... cut by the boundary of round 0 (wave 0) and round 1 (wave 1)
    "tall-waves-L1": (16, 16, "L1"),
    "classes": (16, 16, "L2"),      # one entry per length class, every other id without items
    "dense": (32, 32, "L2"),        # four tiles; tile 0: two chunks, the first of more than four rounds
    "partial": (23, 40, "L2"),      # 3 x 2 tiles, last row 7 rows, last column 8: splats across tiles
    "partial-L1": (23, 40, "L1"),
    "nonfinite": (16, 16, "L2"),    # a NaN colour and an unbounded geometry: no threshold cut
    "wide": (16, 16, "L2"),         # 16-pixel rows: two items each when kBRun < 16
}
# (mean squared error, mean absolute error) of the plain step as int32 bits,
# recorded from the parent build's library (commit e5bebea), not from this one
LOSS_BITS = {
    "items64": (1050273985, 1055850391),
    "items65": (1049729441, 1055343896),
    "items65-L1": (1049729441, 1055343896),
    "items128": (1049579743, 1055191325),
    "items129": (1049489235, 1055042047),
    "tall-row": (1050673928, 1056373107),
    "tall-cross": (1050814159, 1056486152),
    "tall-waves": (1049849511, 1055414627),
    "tall-waves-L1": (1049849511, 1055414627),
    "classes": (1051211781, 1056848464),
    "dense": (1050426230, 1055992705),
    "partial": (1050295464, 1055891309),
    "partial-L1": (1050295464, 1055891309),
    "nonfinite": (1049749624, 1055350808),
    "wide": (1049384085, 1055087673),
}


def _tiles(H, W):
    return (W + 15) // 16, (H + 15) // 16


def _layout(rect, brun=KBRUN):
    """The kernel's item table of a chunk's entries (rank = id order) over the
    whole tile: (entries in slot order, each slot's first item, each slot's
    item count, total).  rect: (x0, x1, y0, y1) inclusive, x0 > x1: none."""
    has = (rect[:, 0] <= rect[:, 1]) & (rect[:, 2] <= rect[:, 3])
    wid = rect[:, 1] - rect[:, 0] + 1
    split = wid > brun
    items = np.where(has, (rect[:, 3] - rect[:, 2] + 1) * np.where(split, 2, 1), 0)
    ilen = np.where(split, (wid + 1) >> 1, wid)
    cls = np.where(items > 0, ((ilen - 1) >> 1) + 1, 0)
    order = np.argsort(-cls, kind="stable")
    n = items[order]
    incl = np.cumsum(n)
    return order, incl - n, n, int(incl[-1]) if len(incl) else 0


def _snake_wave(r):
    return ((r + 1) >> 1) & 1


def _sized(rng, nx, ny, x0, y0):
    """(L row, centre) of an axis-aligned splat whose rectangle is nx columns
    from x0 and ny rows from y0 (before the tile's clipping): the extent
    n / 2 - 0.25 about the middle of the first and last pixel centre, which a
    jitter of 0.08 px leaves 0.17 px from the next count."""
    sx, sy = (nx / 2.0 - 0.26) / K_RECT, (ny / 2.0 - 0.26) / K_RECT
    c = np.array([x0 + (nx - 1) / 2.0, y0 + (ny - 1) / 2.0]) + rng.uniform(-0.08, 0.08, 2)
    return np.array([sx, 0.0, sy], F32), c


def _dot(rng, x, y):
    """A splat too small for any pixel centre: listed in its tile, no rectangle."""
    return np.array([0.1, 0.0, 0.1], F32), np.array([x + 0.5, y + 0.5]) + rng.uniform(-0.05, 0.05, 2)


def _pool(rng, H, W, tile, k):
    """k candidate small splats inside `tile` and their rectangles there."""
    L = S._small_L(rng, k)
    centres = S._one_tile_centres(rng, tile, L, H, W)
    pr = S.project_np(np.tanh(S._raw_xyz(centres, H, W).astype(np.float64)), L.astype(np.float64), H, W)
    ty, tx = divmod(tile, _tiles(H, W)[0])
    return L, centres, S.rect64(pr["xy"], pr["conic"], 16.0 * tx, 16.0 * ty)


def _subset_with_sum(values, target, most):
    """Indices (ascending) of at most `most` of `values` (> 0) that sum to target."""
    best = {0: []}
    for i, v in enumerate(values):
        for s, idx in sorted(best.items(), reverse=True):
            if s + v <= target and len(idx) < most and s + v not in best:
                best[s + v] = idx + [i]
    assert target in best, (target, sorted(best)[-3:])
    return best[target]


def _rows(rect):
    return np.where(rect[:, 0] <= rect[:, 1], rect[:, 3] - rect[:, 2] + 1, 0)


def _stack(parts):
    return np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])


TALL_BEFORE = {"tall-row": 32, "tall-cross": 24, "tall-waves": 56}


def _choose(cid, rng, H, W):
    """(L, centres, faint) of the case's splats in id order; faint: the rows
    whose colours are scaled down (large splats)."""
    base = cid.replace("-L1", "")
    if base.startswith("items"):
        target = int(base[5:])
        L, c, rect = _pool(rng, H, W, 0, 300)
        ok = rng.permutation(np.flatnonzero(_rows(rect) > 0))[:60]
        pick = ok[_subset_with_sum(_rows(rect)[ok], target, 64)]
        return L[pick], c[pick], np.zeros(pick.size, bool)
    if base.startswith("tall"):
        # fillers at least 5 wide (length class 3 and up) come before the tall
        # entry (4 wide: class 2) in the table, whatever their ids
        L, c, rect = _pool(rng, H, W, 0, 300)
        wide = rng.permutation(np.flatnonzero((rect[:, 1] - rect[:, 0] + 1 >= 5) & (_rows(rect) > 0)))[:40]
        pick = wide[_subset_with_sum(_rows(rect)[wide], TALL_BEFORE[base], 20)]
        tall = _sized(rng, 4, 22, 6, -3)  # rows -3 .. 18: the tile's 16
        k = pick.size // 2
        Ls = np.concatenate([L[pick[:k]], tall[0][None], L[pick[k:]]])
        cs = np.concatenate([c[pick[:k]], tall[1][None], c[pick[k:]]])
        faint = np.zeros(pick.size + 1, bool)
        faint[k] = True
        return Ls, cs, faint
    if base == "classes":
        parts = []
        for j, k in enumerate([3, 8, 1, 5, 2, 7, 4, 6]):  # the class of even id 2 j: widths 2 k
            nx, ny = 2 * k, 2 + j % 4
            parts.append(_sized(rng, nx, ny, int(rng.integers(0, 17 - nx)), int(rng.integers(0, 17 - ny))))
            parts.append(_dot(rng, int(rng.integers(0, 15)), int(rng.integers(0, 15))))
        L, c = _stack(parts)
        return L, c, np.arange(16) % 2 == 0
    if base == "dense":
        L = S._small_L(rng, 80)
        return L, S._one_tile_centres(rng, 0, L, H, W), np.zeros(80, bool)
    if base == "partial":
        k = 8
        L = S._small_L(rng, k) * rng.uniform(2.0, 4.0, (k, 1)).astype(F32)
        c = np.stack([rng.uniform(1.0, W - 1.0, k), rng.uniform(1.0, H - 1.0, k)], 1)
        return L, c, np.ones(k, bool)
    if base == "nonfinite":
        L, c, rect = _pool(rng, H, W, 0, 60)
        pick = np.flatnonzero(_rows(rect) > 0)[:18]
        # a tiny splat centred between four pixels: a rectangle, alpha < 1/255
        # at each (its colour becomes NaN on the device); a splat with conic
        # a = 2^44 > 2^40 (cull.h geo_bounded): no rectangle, the chunk's
        # geometry is not bounded
        Ls = np.concatenate([L[pick], np.array([[0.16, 0.0, 0.16], [2.0 ** -22, 0.0, 0.7]], F32)])
        cs = np.concatenate([c[pick], [[9.5, 4.5], [5.3, 11.4]]])
        return Ls, cs, np.zeros(20, bool)
    if base == "wide":
        L, c, rect = _pool(rng, H, W, 0, 60)
        pick = np.flatnonzero(_rows(rect) > 0)[:10]
        parts = [_sized(rng, 20, 6, -2, 1), _sized(rng, 20, 5, -2, 9), _sized(rng, 20, 23, -2, -3)]
        Lw, cw = _stack(parts)
        Ls, cs = np.concatenate([L[pick[:5]], Lw, L[pick[5:]]]), np.concatenate([c[pick[:5]], cw, c[pick[5:]]])
        faint = np.zeros(13, bool)
        faint[5:8] = True
        return Ls, cs, faint
    raise KeyError(cid)


OTHERS = 5  # small splats in each tile that is not tile 0 (dense) / in every tile (partial)


def _build(cid):
    H, W, loss = CASES[cid]
    base = cid.replace("-L1", "")
    rng = np.random.default_rng(5200 + sorted(CASES).index(base))
    L, centres, faint = _choose(cid, rng, H, W)
    k = L.shape[0]
    col = rng.uniform(-0.3, 1.0, (k, 3)) * 20.0 / max(k, 12)
    col[faint] *= 0.25
    ntile = k
    tbx, tby = _tiles(H, W)
    if base in ("dense", "partial"):
        for t in range(tbx * tby):
            if base == "partial" or t != 0:
                Lo = S._small_L(rng, OTHERS)
                L = np.concatenate([L, Lo])
                centres = np.concatenate([centres, S._one_tile_centres(rng, t, Lo, H, W)])
                col = np.concatenate([col, rng.uniform(-0.3, 1.0, (OTHERS, 3)) * 20.0 / (OTHERS + 4)])
    if base == "partial":  # ids shuffled: the large splats anywhere in the tiles' lists
        perm = rng.permutation(L.shape[0])
        L, centres, col = L[perm], centres[perm], col[perm]
    p = S._params(H, W, S._raw_xyz(centres, H, W), L, col.astype(F32), 93, loss=loss)
    p["claims"].update(ids=np.arange(ntile))
    return p


def _case(cid):
    """(p, r) of sum_cases.fused_case for this module's builder: the same margin
    loop, cache and error measures as the shared cases."""
    key = "pool-" + cid
    if key not in S._fused_cache:
        shared = S._build_fused
        S._build_fused = lambda _: _build(cid)
        try:
            S.fused_case(key)
        finally:
            S._build_fused = shared
    return S.fused_case(key)


def _gpu_params(cid):
    """What the kernels get: the case, with the non-finite colour in place."""
    p, _ = _case(cid)
    if cid != "nonfinite":
        return p
    q = dict(p)
    q["feat"] = p["feat"].copy()
    q["feat"][18, 1] = np.nan
    return q


def _tile_rects(p, r, tile):
    """(ids, rectangles) of a tile's entries, in rank (= id) order."""
    H, W = p["H"], p["W"]
    tbx, tby = _tiles(H, W)
    ids = S.bin_np(r["proj"]["box"], tbx, tby)[tile].astype(np.int64)
    ty, tx = divmod(tile, tbx)
    return ids, S.rect64(r["proj"]["xy"][ids], r["proj"]["conic"][ids], 16.0 * tx, 16.0 * ty)


def _one_tile_splats(r):
    b = r["proj"]["box"]
    return (b[:, 1] - b[:, 0]) * (b[:, 3] - b[:, 2]) == 1


def _claims(cid):
    """Assert on the reference what the case is named for."""
    p, r = _case(cid)
    H, W = p["H"], p["W"]
    base = cid.replace("-L1", "")
    ids, rect = _tile_rects(p, r, 0)
    order, off, n, total = _layout(rect)
    print(f"{cid}: tile 0 holds {ids.size} entries, {total} items, kBRun {KBRUN}")
    if base not in ("dense", "partial"):
        np.testing.assert_array_equal(ids, np.arange(p["xyz"].shape[0]))  # one tile, every splat listed
        assert ids.size <= 64  # one chunk
        assert _one_tile_splats(r).all()
    # the slots with items are a prefix of the table
    assert (n[:np.count_nonzero(n)] > 0).all()
    if base.startswith("items"):
        assert total == int(base[5:])
    if base.startswith("tall"):
        assert KBRUN >= 4  # the tall entry's rows are whole items
        tall =int(np.flatnonzero((rect[:, 2] == 0) & (rect[:, 3] == 15))[0])
        k = int(np.flatnonzero(order == tall)[0])
        assert rect[tall, 1] - rect[tall, 0] + 1 == 4 and n[k] == 16 and off[k] == TALL_BEFORE[base]
        first, last = off[k], off[k] + 15
        if base == "tall-row":
            assert first % 16 == 0
        if base == "tall-cross":
            assert first // 16 != last // 16 and first // 64 == last // 64
        if base == "tall-waves":
            assert (first // 64, last // 64) == (0, 1) and _snake_wave(0) != _snake_wave(1)
    if base == "classes":
        wid = rect[:, 1] - rect[:, 0] + 1
        assert (_rows(rect)[1::2] == 0).all() and (_rows(rect)[0::2] > 0).all()
        np.testing.assert_array_equal((wid[0::2] - 1) >> 1, np.array([3, 8, 1, 5, 2, 7, 4, 6]) - 1)
        np.testing.assert_array_equal(order[:8], 2 * np.array([1, 5, 7, 3, 6, 0, 4, 2]))  # classes 8 .. 1
        np.testing.assert_array_equal(order[8:], np.arange(1, 16, 2))  # no items: id order, last
    if base == "dense":
        assert ids.size == 80 and _one_tile_splats(r).all()
        np.testing.assert_array_equal(np.delete(r["c"]["counts"], 0), OTHERS)
        first = _layout(rect[:64])[3]
        assert first > 256 and _layout(rect[64:])[3] > 0  # more than four rounds; a second chunk with items
    if base == "partial":
        tbx, tby = _tiles(H, W)
        many = ~_one_tile_splats(r) & r["proj"]["ok"]
        assert many.sum() >= 4 and (r["c"]["counts"] > OTHERS).all()
        below = right = 0
        for t in range(tbx * tby):
            ty, tx = divmod(t, tbx)
            _, rc = _tile_rects(p, r, t)
            has = rc[:, 0] <= rc[:, 1]
            below += int((has & (rc[:, 3] + 16 * ty >= H)).sum())
            right += int((has & (rc[:, 1] + 16 * tx >= W)).sum())
        assert below >= 3 and right >= 3  # rectangle rows below the image, columns right of it
    if base == "nonfinite":
        assert rect[18, 0] <= rect[18, 1] and _rows(rect)[18] > 0  # the NaN-to-be has items ...
        for t in r["fwd"]["tiles"]:  # ... and passes the cut nowhere: its colour enters no sum
            assert not t["keep"][:, t["g"] == 18].any()
        assert r["proj"]["conic"][19, 0] > 2.0 ** 41 and _rows(rect)[19] == 0
        feat = _gpu_params(cid)["feat"]
        assert np.isnan(feat[18]).sum() == 1 and np.isfinite(np.delete(feat, 18, 0)).all()
    if base == "wide":
        wid = rect[:, 1] - rect[:, 0] + 1
        full = np.flatnonzero(wid == 16)
        assert full.size == 3 and sorted(_rows(rect)[full].tolist()) == [5, 6, 16]
        per_row = 2 if 16 > KBRUN else 1
        k = np.flatnonzero(np.isin(order, full))
        np.testing.assert_array_equal(n[k], _rows(rect)[order[k]] * per_row)
        assert total > 64
    return order, off, n, total


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _op_counts(p):
    from gsvc_amd import ops
    from gsvc_amd.utils import bin_and_sort_for_raster
    H, W = p["H"], p["W"]
    means, L, _ = S.activated32(p)
    n = means.shape[0]
    tb = (*_tiles(H, W), 1)
    xys, depths, radii, conics, nth = ops.project_gaussians_2d_forward(n, E.T(means), E.T(L), H, W, tb, 0.01)
    _, _, bins = bin_and_sort_for_raster(n, xys, depths, radii, nth, tb)
    return bins[:, 1] - bins[:, 0]


@pytest.mark.parametrize("cid", list(CASES))
def test_case_is_what_it_claims(cuda, cid):
    p, r = _case(cid)
    _claims(cid)
    np.testing.assert_array_equal(E.N(_op_counts(p)), r["c"]["counts"])  # the kernels' binning agrees


def _check(cid, what, render, losses, g):
    E._check_fused("pool-" + cid, what, render, losses, g)


@pytest.mark.parametrize("cid", list(CASES))
def test_gradients_only_step_against_float64(cuda, cid):
    pg = _gpu_params(cid)
    with E.deterministic():
        render, losses, g = E._step(pg, cuda)
        torch.cuda.synchronize()
    assert bool(torch.isfinite(render).all()) and bool(torch.isfinite(losses).all())
    assert bool(torch.isfinite(g).all())
    _check(cid, "grads-only", render, losses, g)
    img = E._model(pg, cuda, fused_train=False)()["render"]
    assert torch.equal(_bits(render), _bits(img[0]))  # the frame render's bits


def _train(pg, dev, carry, steps, **kw):
    from gsvc_amd import train as TR
    old = TR.CARRY_BINS
    TR.CARRY_BINS = carry
    try:
        m = E._model(pg, dev, fused_train=True, **kw)
        gt = E.T(pg["gt"]).view(1, 3, pg["H"], pg["W"])
        out = [m.train_iter(gt, it) for it in range(1, steps + 1)]
        torch.cuda.synchronize()
        assert m.fused_steps == steps
        return m, out
    finally:
        TR.CARRY_BINS = old


@pytest.mark.parametrize("cid", list(CASES))
def test_adan_step_against_float64(cuda, cid):
    """train_iter with lr 0: adan.h stores neg_pre_grad = -g, the step's gradient."""
    p, r = _case(cid)
    pg = _gpu_params(cid)
    with E.deterministic():
        m, out = _train(pg, cuda, True, 1, lr=0.0)
        with torch.no_grad():
            render = m()["render"][0].clone()
    names = ["_xyz", "_cholesky", "_features_dc"]
    g = torch.cat([-m.optimizer.state[getattr(m, k)]["neg_pre_grad"] for k in names]
                  + [torch.zeros(len(p["xyz"]), 1, device=cuda)], 1)
    loss, psnr = out[0]
    mse = 10.0 ** (-float(psnr) / 10.0)
    assert bool(torch.isfinite(g).all())
    losses = [mse, float(loss)] if p["loss"] == "L1" else [float(loss), r["losses"][1]]
    _check(cid, "train_iter", render, np.array(losses), g)


@pytest.mark.parametrize("cid", list(CASES))
def test_carried_bins_equal_reprojected_bitwise(cuda, cid):
    pg = _gpu_params(cid)
    with E.deterministic():
        ma, oa = _train(pg, cuda, True, 3)
        mb, ob = _train(pg, cuda, False, 3)
    la, lb = [(float(a), float(b)) for a, b in oa], [(float(a), float(b)) for a, b in ob]
    print(cid, "losses", la, lb)
    assert la == lb and all(np.isfinite(v) for pair in la for v in pair)
    for k, v in ma.state_dict().items():
        assert torch.equal(_bits(v), _bits(mb.state_dict()[k])), k
    for pa, pb in zip(ma.optimizer.param_groups[0]["params"], mb.optimizer.param_groups[0]["params"]):
        for key in ("exp_avg", "exp_avg_sq", "exp_avg_diff", "neg_pre_grad"):
            assert torch.equal(_bits(ma.optimizer.state[pa][key]), _bits(mb.optimizer.state[pb][key])), key


@pytest.mark.parametrize("cid", list(CASES))
def test_deterministic_repeats_equal_plain_and_recorded_losses(cuda, cid):
    """Two deterministic runs agree bit for bit.  A splat in one tile gets one
    flush's sum onto zero, by an atomic add (plain) or into its one slot
    (deterministic): the same bits.  The plain step's losses and render carry
    the parent build's bits (LOSS_BITS)."""
    p, r = _case(cid)
    pg = _gpu_params(cid)
    ra, la, ga = E._step(pg, cuda)
    torch.cuda.synchronize()
    with E.deterministic():
        rb, lb, gb = E._step(pg, cuda)
        rc, lc, gc = E._step(pg, cuda)
        torch.cuda.synchronize()
    bits = tuple(int(v) for v in _bits(la).tolist())
    print(f'LOSS_BITS    "{cid}": ({bits[0]}, {bits[1]}),')
    for x, y in ((rb, rc), (lb, lc), (gb, gc)):
        assert torch.equal(_bits(x), _bits(y))
    assert torch.equal(_bits(la), _bits(lb))
    assert torch.equal(_bits(ra), _bits(rb))
    one = torch.from_numpy(_one_tile_splats(r)).to(ga.device)
    assert int(one.sum()) >= 5
    assert torch.equal(_bits(ga[one]), _bits(gb[one]))
    assert bits == LOSS_BITS[cid]
