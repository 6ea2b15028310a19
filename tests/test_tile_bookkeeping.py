"""The training tile kernel's bookkeeping (train.hip, train_tile_band_kernel;
DESIGN.md section 6): the chunk's facts decided once where the chunk is staged
(every colour finite, every geometry bounded -- which blend and which backward
alpha cut the chunk takes), the lane-group lists built with lane counts, the
loss gradients under one branch on the loss kind.

One 72x40 frame per case (width divisible by 4: the 16-byte target loads; 5 x 3
tiles, the right tiles 8 columns and the bottom tiles 8 rows) with the case's
content in the interior tile 6, and one 70x40 frame (the 4-byte target loads).
Each case is built from sum_cases' placement helpers, registered with
sum_cases.fused_case (so its float64 reference, its decision margins and the
error measures are the shared ones) and asserted to be what it claims with the
op path's projection and binning.  Every case is held to

* sum_cases.BARS against the float64 reference: both losses,
  the render and the nine gradient columns, for one gradients-only
  train_step_sum call and for one train_iter step with the Adan update (lr 0:
  the gradient is read off the optimizer state), under the deterministic
  backward;
* bitwise, three real train_iter steps with carried bins against re-projected
  ones under the deterministic backward (the same kernel, the candidates in two
  orders);
* bitwise, the grouped forward against Knob.TILE_NO_GROUPS = 1 in the diagnostic
  library: losses and render.

The two entries with a NaN and an infinite colour pass the alpha cut at no
pixel (asserted on the reference's kept pairs), so the reference -- which
multiplies every pair's colour by its weight, 0 x NaN included -- is taken with
finite colours for them; the kernels get the non-finite ones, and everything
they return must still be finite and within the bars.
"""
import numpy as np
import pytest
import torch

import sum_cases as S
import test_sum_edges as E
from conftest import knobs
from gsvc_amd.knobs import Knob

F32 = np.float32
TILE6 = 6  # tile (1, 1) of the 5 x 3: full, interior
BG = 24    # background splats over the whole frame (they reach the partial edge tiles)

# case -> (W, small splats placed in tile 6, the range its entry count must lie in)
CASES = {
    "le32": (72, 12, (2, 32)),
    "le64": (72, 40, (33, 64)),
    "le256": (72, 100, (65, 256)),
    "gt256": (72, 300, (257, 10 ** 6)),
    "nonfinite": (72, 20, (2, 64)),
    "unbounded": (72, 20, (2, 64)),
    "wide-row": (72, 20, (2, 64)),
    "band1": (72, 20, (2, 64)),
    "w70": (70, 20, (2, 64)),
}
# the special entry of a case: Cholesky row and centre (tile 6 spans x, y in [16, 32))
SPECIAL = {
    "nonfinite": [((0.16, 0.0, 0.16), (24.5, 20.5)), ((0.16, 0.0, 0.16), (21.5, 27.5))],
    "unbounded": [((10.0 * 2.0 ** -25, 0.0, 0.8), (24.5, 24.5))],
    "wide-row": [((3.5, 0.0, 0.7), (24.0, 22.3))],
    "band1": [((0.6, 0.0, 0.6), (24.2, 28.1))],
}
H = 40


def _build(cid):
    W, k, _ = CASES[cid]
    rng = np.random.default_rng(900 + sorted(CASES).index(cid))
    L = S._small_L(rng, k)
    centres = S._one_tile_centres(rng, TILE6, L, H, W)
    col = rng.uniform(-0.3, 1.0, (k, 3)) * 20.0 / k
    Lb = (rng.random((BG, 3)) + np.array([0.5, 0.0, 0.5])).astype(F32)
    cb = np.stack([rng.uniform(0.5, W - 0.5, BG), rng.uniform(0.5, H - 0.5, BG)], 1)
    colb = rng.uniform(-0.3, 1.0, (BG, 3)) * 0.1
    sp = SPECIAL.get(cid, [])
    Ls = np.array([s[0] for s in sp], F32).reshape(-1, 3)
    cs = np.array([s[1] for s in sp], np.float64).reshape(-1, 2)
    cols = rng.uniform(0.2, 0.6, (len(sp), 3))
    L, centres, col = np.concatenate([L, Lb, Ls]), np.concatenate([centres, cb, cs]), np.concatenate([col, colb, cols])
    special = np.arange(k + BG, k + BG + len(sp))
    perm = rng.permutation(L.shape[0])  # ids in no order of place
    p = S._params(H, W, S._raw_xyz(centres[perm], H, W), L[perm], col[perm].astype(F32), 81)
    p["claims"].update(special=np.sort(np.argsort(perm)[special]))
    return p


def _case(cid):
    """(p, r) of sum_cases.fused_case for this module's builder: the same margin
    loop, cache and error measures as the shared cases."""
    if cid not in S._fused_cache:
        shared = S._build_fused
        S._build_fused = _build
        try:
            S.fused_case(cid)
        finally:
            S._build_fused = shared
    return S.fused_case(cid)


def _gpu_params(cid):
    """What the kernels get: the case, with the non-finite colours in place."""
    p, _ = _case(cid)
    if cid != "nonfinite":
        return p
    q = dict(p)
    q["feat"] = p["feat"].copy()
    a, b = p["claims"]["special"]
    q["feat"][a, 1] = np.nan
    q["feat"][b, 2] = np.inf
    return q


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _op_binning(p, dev):
    """The op path's projection and binning of the case: per-tile counts, the
    tile's ids, float32 centres and conics."""
    from gsvc_amd import ops
    from gsvc_amd.utils import bin_and_sort_for_raster
    means, L, _ = S.activated32(p)
    n = means.shape[0]
    tb = ((p["W"] + 15) // 16, (p["H"] + 15) // 16, 1)
    xys, depths, radii, conics, nth = ops.project_gaussians_2d_forward(n, E.T(means), E.T(L), p["H"], p["W"],
                                                                       tb, 0.01)
    _, gids, bins = bin_and_sort_for_raster(n, xys, depths, radii, nth, tb)
    bins, gids = E.N(bins), E.N(gids)
    return bins[:, 1] - bins[:, 0], gids[bins[TILE6, 0]:bins[TILE6, 1]], E.N(xys), E.N(conics)


@pytest.mark.parametrize("cid", list(CASES))
def test_case_is_what_it_claims(cuda, cid):
    p, r = _case(cid)
    counts, ids, xys, conics = _op_binning(p, cuda)
    lo, hi = CASES[cid][2]
    print(f"{cid}: tile {TILE6} holds {counts[TILE6]} entries; frame counts {counts.tolist()}")
    assert lo <= counts[TILE6] <= hi
    np.testing.assert_array_equal(counts, r["c"]["counts"])  # the reference bins alike
    assert counts[4::5].sum() > 0 and counts[10:].sum() > 0  # the partial right / bottom tiles hold entries
    sp = p["claims"]["special"]
    assert np.isin(sp, ids).all()
    rect = S.rect64(xys[sp].astype(np.float64), conics[sp].astype(np.float64), 16.0, 16.0)
    if cid == "nonfinite":
        feat = _gpu_params(cid)["feat"]
        assert np.isnan(feat[sp[0]]).sum() == 1 and np.isinf(feat[sp[1]]).sum() == 1
        assert np.isfinite(np.delete(feat, sp, 0)).all()
        assert (rect[:, 0] <= rect[:, 1]).all()  # each reaches a lane group: its list walks it
        for t in r["fwd"]["tiles"]:  # ... and passes the cut nowhere: its colour enters no sum
            assert not t["keep"][:, np.isin(t["g"], sp)].any()
    if cid == "unbounded":
        assert 0.5 * conics[sp[0], 0] >= 2.0 ** 40  # cull.h geo_bounded: |a / 2| < 2^40
        assert np.isfinite(p["feat"]).all()
        others = np.setdiff1d(ids, sp)
        assert (np.abs(conics[others]) < 2.0 ** 40).all() and (np.abs(xys[others]) < 2.0 ** 20).all()
    if cid == "wide-row":
        assert rect[0, 1] - rect[0, 0] + 1 > 10
    if cid == "band1":
        assert rect[0, 2] >= 8 and rect[0, 2] <= rect[0, 3]


@pytest.mark.parametrize("cid", list(CASES))
def test_gradients_only_step_against_float64(cuda, cid):
    pg = _gpu_params(cid)
    with E.deterministic():
        render, losses, g = E._step(pg, cuda)
        torch.cuda.synchronize()
    assert bool(torch.isfinite(render).all()) and bool(torch.isfinite(losses[:2]).all())
    assert bool(torch.isfinite(g).all())
    E._check_fused(cid, "grads-only", render, losses, g)


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
    assert bool(torch.isfinite(g).all())
    E._check_fused(cid, "train_iter", render, np.array([float(loss), r["losses"][1]]), g)
    assert abs(10.0 ** (-float(psnr) / 10.0) - float(loss)) <= 1e-12 * float(loss)


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
def test_grouped_forward_equals_ungrouped_bitwise(cuda, cid):
    """Both in the diagnostic library: its grouped forward (the product's code)
    against Knob.TILE_NO_GROUPS = 1, the band-mask walk."""
    from gsvc_amd import _lib
    pg = _gpu_params(cid)
    with E.deterministic():
        with _lib.diagnostic():
            ra, la, ga = E._step(pg, cuda)
            torch.cuda.synchronize()
        with knobs((Knob.TILE_NO_GROUPS, 1)):
            rb, lb, gb = E._step(pg, cuda)
            torch.cuda.synchronize()
    print(cid, "losses", la.tolist(), lb.tolist())
    assert torch.equal(_bits(la), _bits(lb))
    assert torch.equal(_bits(ra), _bits(rb))
    assert torch.equal(_bits(ga), _bits(gb))


def test_product_library_keeps_its_four_tile_instances():
    """No GPU: the built product library still has exactly the four band tile
    kernel instances, each within 64 VGPRs, no scratch and 10240 bytes of LDS --
    the check of tests/test_tile_resident.py itself."""
    import test_tile_resident as R
    R.test_product_tile_instances_fit_their_registers()
