"""The backward rounds of the training tile kernel (train.hip,
train_tile_band_kernel): an item's sorted slot counted from
one ballot of the run starts (the entries without items in the band ranked
last, a class of their own), no validity selects under the threshold cut, the
loss sums by DPP.

One 28x48 frame per case (3 x 2 tiles; the bottom tiles hold 12 rows, so their
second band has four rows inside the image and four below it).  A case's
content is small splats, each inside one tile, drawn from a pool and chosen by
the rows their alpha >= 1/255 rectangle (sum_cases.rect64) takes in each
8-row band -- an item is one rectangle row -- so that a band of the content
tile has exactly the item count, or the arrangement of entries, the case
names; every other tile gets a few splats of its own.  `_layout` restates the
kernel's item layout (entries by length class, longest first, id order within a
class; the entries without items hold none) and `test_case_is_what_it_claims`
asserts each claim on the case's float64 reference after its margin loop.

Each case is registered with sum_cases.fused_case and held to

* sum_cases.BARS against the float64 reference: both losses, the render and the
  nine gradient columns, for a gradients-only train_step_sum call and for a
  train_iter step with the Adan update (lr 0), under the deterministic backward;
* bitwise, three train_iter steps with carried bins against re-projected ones;
* bitwise, the deterministic against the plain backward: every splat of these
  frames lies in one tile, so its gradient is one flush's sum either way;
* bitwise, the two losses of the plain step against LOSS_BITS, recorded from the
  parent build (the shuffle butterfly): the DPP sums add in the same order.
"""
import numpy as np
import pytest
import torch

import sum_cases as S
import test_sum_edges as E

pytestmark = pytest.mark.gpu

F32 = np.float32
H, W = 28, 48
MAIN, BOTTOM = 1, 4  # content tiles: (tx 1, ty 0), 16 rows; (tx 1, ty 1), 12 rows
OTHERS = 5           # splats in each tile that is not the case's content tile

# case -> (content tile, loss); what each claims: _claims
CASES = {
    "items64": (MAIN, "L2"),       # band 0: exactly 64 items, one round
    "items65": (MAIN, "L2"),       # band 0: 65, a one-item second round
    "items65-L1": (MAIN, "L1"),
    "rounds3": (MAIN, "L2"),       # band 0: three rounds, runs across both 64-item boundaries
    "alternate": (MAIN, "L2"),     # by id, entries of band 0 only and of band 1 only in turn
    "band-empty": (MAIN, "L2"),    # every entry in band 0: band 1 has entries and no item
    "bottom": (BOTTOM, "L2"),      # rectangle rows below the image
    "bottom-L1": (BOTTOM, "L1"),
    "nonfinite": (MAIN, "L2"),     # one NaN colour: the chunk keeps the alpha test as written
}
# (mean squared error, mean absolute error) of the plain step as int32 bits,
# recorded from the parent build's library (commit 2387a63), not from this one
LOSS_BITS = {
    "items64": (1051025368, 1056568629),
    "items65": (1050816955, 1056347587),
    "items65-L1": (1050816955, 1056347587),  # (both sums are taken under either loss)
    "rounds3": (1050666508, 1056241290),
    "alternate": (1050952403, 1056456006),
    "band-empty": (1050851846, 1056395419),
    "bottom": (1050625501, 1056191284),
    "bottom-L1": (1050625501, 1056191284),
    "nonfinite": (1050722270, 1056234998),
}


def _tile_origin(t):
    ty, tx = divmod(t, (W + 15) // 16)
    return 16.0 * tx, 16.0 * ty


def _band_rows(rect, band):
    """Rows of each rectangle (x0, x1, y0, y1; x0 > x1: none) inside a band."""
    y0 = np.maximum(rect[:, 2], 8 * band)
    y1 = np.minimum(rect[:, 3], 8 * band + 7)
    return np.where((rect[:, 0] <= rect[:, 1]) & (y0 <= y1), y1 - y0 + 1, 0)


def _layout(rect, band):
    """The kernel's item layout of a chunk's entries (rank = id order) in one
    band: (entries in slot order, each slot's first item, total).  Rows are at
    most 16 wide: an item is a whole row."""
    items = _band_rows(rect, band)
    wid = rect[:, 1] - rect[:, 0] + 1
    cls = np.where(items == 0, 0, np.where(wid >= 9, 4, np.where(wid >= 7, 3, np.where(wid >= 5, 2, 1))))
    order = np.argsort(-cls, kind="stable")
    incl = np.cumsum(items[order])
    return order, incl - items[order], int(incl[-1]) if len(incl) else 0


def _pool(rng, tile, k):
    """k candidate small splats inside `tile` and their rectangles."""
    L = S._small_L(rng, k)
    centres = S._one_tile_centres(rng, tile, L, H, W)
    xyz = S._raw_xyz(centres, H, W)
    pr = S.project_np(np.tanh(xyz.astype(np.float64)), L.astype(np.float64), H, W)
    return L, centres, S.rect64(pr["xy"], pr["conic"], *_tile_origin(tile))


def _subset_with_sum(values, target, most):
    """Indices (ascending) of at most `most` of `values` (> 0) that sum to target."""
    best = {0: []}
    for i, v in enumerate(values):
        for s, idx in sorted(best.items(), reverse=True):
            if s + v <= target and len(idx) < most and s + v not in best:
                best[s + v] = idx + [i]
    assert target in best, (target, sorted(best)[-3:])
    return best[target]


def _choose(cid, rng, tile):
    """The content tile's splats: rows of (L, centre), in id order."""
    L, c, rect = _pool(rng, tile, 400)
    r0, r1 = _band_rows(rect, 0), _band_rows(rect, 1)
    if cid.startswith("items") or cid == "rounds3":
        target = {"items64": 64, "items65": 65, "items65-L1": 65, "rounds3": 150}[cid]
        for _ in range(200):
            ok = rng.permutation(np.flatnonzero(r0 > 0))[:60]
            pick = ok[_subset_with_sum(r0[ok], target, 64)]
            order, off, _ = _layout(rect[pick], 0)
            n = r0[pick][order]
            if cid != "rounds3" or all(((off < e) & (off + n > e)).any() for e in (64, 128)):
                break
        else:
            raise AssertionError("no subset with a run across both round boundaries")
    elif cid == "alternate":
        a, b = np.flatnonzero((r0 > 0) & (r1 == 0))[:12], np.flatnonzero((r0 == 0) & (r1 > 0))[:12]
        pick = np.stack([a, b], 1).reshape(-1)  # ids 0, 2, ...: band 0 only; 1, 3, ...: band 1 only
    elif cid == "band-empty":
        pick = np.flatnonzero((r0 > 0) & (r1 == 0))[:14]
    elif cid.startswith("bottom"):
        below = rect[:, 3] + 16 >= H  # the rectangle's last row is below the image
        pick = np.concatenate([np.flatnonzero(below)[:10], np.flatnonzero(~below)[:8]])
        pick = pick[rng.permutation(pick.size)]
    elif cid == "nonfinite":
        pick = np.flatnonzero(r0 + r1 > 0)[:18]
    return L[pick], c[pick]


def _build(cid):
    tile, loss = CASES[cid]
    rng = np.random.default_rng(4100 + sorted(CASES).index(cid.replace("-L1", "")))
    L, centres = _choose(cid, rng, tile)
    k = L.shape[0]
    col = rng.uniform(-0.3, 1.0, (k, 3)) * 20.0 / k
    if cid == "nonfinite":
        # a tiny splat centred between four pixels: a rectangle, and alpha < 1/255 at each
        L = np.concatenate([L, np.array([[0.16, 0.0, 0.16]], F32)])
        centres = np.concatenate([centres, [[24.5, 4.5]]])
        col = np.concatenate([col, rng.uniform(0.2, 0.6, (1, 3))])
    ntile = L.shape[0]
    for t in range(6):
        if t != tile:
            Lo = S._small_L(rng, OTHERS)
            L = np.concatenate([L, Lo])
            centres = np.concatenate([centres, S._one_tile_centres(rng, t, Lo, H, W)])
            col = np.concatenate([col, rng.uniform(-0.3, 1.0, (OTHERS, 3)) * 20.0 / OTHERS])
    # the content tile's splats keep the lowest ids, in the order chosen; ids are ranks
    p = S._params(H, W, S._raw_xyz(centres, H, W), L, col.astype(F32), 91, loss=loss)
    p["claims"].update(tile=tile, ids=np.arange(ntile))
    return p


def _case(cid):
    """(p, r) of sum_cases.fused_case for this module's builder: the same margin
    loop, cache and error measures as the shared cases."""
    key = "rounds-" + cid
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
    q["feat"][p["claims"]["ids"][-1], 1] = np.nan
    return q


def _claims(cid):
    """Assert on the reference what the case is named for; returns the per-band
    (order, off, total) of the content tile."""
    p, r = _case(cid)
    tile, ids = p["claims"]["tile"], p["claims"]["ids"]
    counts = r["c"]["counts"]
    np.testing.assert_array_equal(np.delete(counts, tile), OTHERS)  # one tile each
    assert counts[tile] == ids.size <= 64  # one chunk
    pr = r["proj"]
    rect = S.rect64(pr["xy"][ids], pr["conic"][ids], *_tile_origin(tile))
    lay = [_layout(rect, b) for b in (0, 1)]
    tot = [l[2] for l in lay]
    rows = [_band_rows(rect, b) for b in (0, 1)]
    print(f"{cid}: {ids.size} entries, items per band {tot}")

    def crosses(band, step):  # a run with items on both sides of a multiple of `step`
        order, off, _ = lay[band]
        n = rows[band][order]
        return bool(((n > 0) & (off // step != (off + n - 1) // step)).any())

    if cid == "items64":
        assert tot[0] == 64
    if cid.startswith("items65"):
        assert tot[0] == 65
    if cid == "rounds3":
        assert 128 < tot[0] <= 192
        order, off, _ = lay[0]
        n = rows[0][order]
        for edge in (64, 128):  # a run on both sides of each round boundary
            assert ((off < edge) & (off + n > edge)).any()
    if cid in ("items64", "rounds3"):
        assert crosses(0, 16)  # ... and of a 16-lane row inside a round
    if cid == "alternate":
        assert (rows[0][0::2] > 0).all() and (rows[0][1::2] == 0).all()
        assert (rows[1][0::2] == 0).all() and (rows[1][1::2] > 0).all()
    if cid == "band-empty":
        assert tot[0] > 0 and tot[1] == 0
    if cid.startswith("bottom"):
        below = rect[:, 3] + 16 >= H
        assert below.sum() >= 5 and (~below).sum() >= 5 and tot[1] > 0
    if cid == "nonfinite":
        assert (rect[-1, 0] <= rect[-1, 1]) and rows[0][-1] > 0  # it has items ...
        for t in r["fwd"]["tiles"]:  # ... and passes the cut nowhere: its colour enters no sum
            assert not t["keep"][:, t["g"] == ids[-1]].any()
        feat = _gpu_params(cid)["feat"]
        assert np.isnan(feat[ids[-1]]).sum() == 1 and np.isfinite(np.delete(feat, ids[-1], 0)).all()
    if cid in ("items64", "band-empty"):
        assert max(tot) <= 64  # single rounds
    return lay


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


@pytest.mark.parametrize("cid", list(CASES))
def test_case_is_what_it_claims(cuda, cid):
    p, r = _case(cid)
    _claims(cid)
    counts = E.N(_op_counts(p))
    np.testing.assert_array_equal(counts, r["c"]["counts"])  # the kernels' binning agrees


def _op_counts(p):
    from gsvc_amd import ops
    from gsvc_amd.utils import bin_and_sort_for_raster
    means, L, _ = S.activated32(p)
    n = means.shape[0]
    tb = ((W + 15) // 16, (H + 15) // 16, 1)
    xys, depths, radii, conics, nth = ops.project_gaussians_2d_forward(n, E.T(means), E.T(L), H, W, tb, 0.01)
    _, _, bins = bin_and_sort_for_raster(n, xys, depths, radii, nth, tb)
    return bins[:, 1] - bins[:, 0]


def _check(cid, what, render, losses, g):
    E._check_fused("rounds-" + cid, what, render, losses, g)


@pytest.mark.parametrize("cid", list(CASES))
def test_gradients_only_step_against_float64(cuda, cid):
    pg = _gpu_params(cid)
    with E.deterministic():
        render, losses, g = E._step(pg, cuda)
        torch.cuda.synchronize()
    assert bool(torch.isfinite(render).all()) and bool(torch.isfinite(losses).all())
    assert bool(torch.isfinite(g).all())
    _check(cid, "grads-only", render, losses, g)


def _train(pg, dev, carry, steps, **kw):
    from gsvc_amd import train as TR
    old = TR.CARRY_BINS
    TR.CARRY_BINS = carry
    try:
        m = E._model(pg, dev, fused_train=True, **kw)
        gt = E.T(pg["gt"]).view(1, 3, H, W)
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
def test_deterministic_equals_plain_and_recorded_losses(cuda, cid):
    """Every splat lies in one tile, so the plain backward's one atomic add per
    splat and sum onto zero is the deterministic backward's one slot; the plain
    step's losses carry the parent build's bits (LOSS_BITS)."""
    pg = _gpu_params(cid)
    ra, la, ga = E._step(pg, cuda)
    torch.cuda.synchronize()
    with E.deterministic():
        rb, lb, gb = E._step(pg, cuda)
        torch.cuda.synchronize()
    bits = tuple(int(v) for v in _bits(la).tolist())
    print(f'LOSS_BITS "{cid}": ({bits[0]}, {bits[1]}),')
    assert torch.equal(_bits(la), _bits(lb))
    assert torch.equal(_bits(ra), _bits(rb))
    assert torch.equal(_bits(ga), _bits(gb))
    assert bits == LOSS_BITS[cid]
