"""Binning, render and the fused training step on the tile grids of
tests/grid_cases.py: tile counts on both sides of the scan chunk (8192 tiles,
binning.h scan_tile_counts), of the loss workgroup's trip (8192 tiles,
train.hip publish_loss), of each radix-sort width (0, 1, 8, 9, 13..17 bits),
with xcd_remap / xcd_runs tails other than 0 and 96, and past one resident
round of tile workgroups.  Binning is exact against the integer reference;
images, losses and gradients go against the float64 references of
sum_cases.py under its bars (sum_cases.GRID_BARS where the wide frames' input
rounding exceeds them), every figure printed before it is asserted (``SUM-ERR``
lines; pytest -s shows them)."""
import math

import numpy as np
import pytest
import torch

import grid_cases as G
import sum_cases as S
from conftest import knobs
from gsvc_amd.knobs import Knob
from test_sum_edges import N, T, _model, _step, deterministic, tile_kernel  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu


def _report(cid, what, name, value, bar):
    print(f"SUM-ERR {cid} {what} {name} {value:.3e} bar {bar:.3e}")


# ---------------------------------------------------------------- binning, exact
def _grid_dev(grid):
    g = G.bin_grid(*grid)
    return g, g["ref"], (g["tbx"], g["tby"], 1), T(g["xys"]), T(g["radii"]), T(g["depths"])


@pytest.mark.parametrize("cap", [0, 256])
@pytest.mark.parametrize("grid", G.BIN_GRIDS, ids=G.BIN_IDS)
def test_bin_tiles_counted(cuda, grid, cap):
    """gsvc_bin_tiles_counted (count, scan, fill, segment sort, overflow
    rebuild): tile_bins, M and every tile's ids -- its first 256 when capped --
    exact; no overflow at a capacity of exactly the entries kept; a second call
    gives the same."""
    from gsvc_amd import ops
    g, ref, tb, xys, radii, _ = _grid_dev(grid)
    capacity = ref["M_capped"] if cap else ref["M"]
    runs = [ops.bin_tiles_counted(g["n"], xys, radii, tb, capacity, cap) for _ in range(2)]
    gids, bins, meta = runs[0]
    assert N(meta).tolist() == [ref["M"], 0]
    np.testing.assert_array_equal(N(bins), ref["bins_capped" if cap else "bins"])
    np.testing.assert_array_equal(N(gids)[:capacity], ref["gids_capped" if cap else "gids"])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("grid", G.BIN_GRIDS, ids=G.BIN_IDS)
def test_bin_and_sort_tiles(cuda, grid):
    """gsvc_compute_cumulative_intersects and gsvc_bin_and_sort_tiles (the
    radix sort on bits_for(tiles) bits: the copy branch at 0, one to three
    passes) with the expanded int64 keys."""
    from gsvc_amd import ops
    g, ref, tb, xys, radii, depths = _grid_dev(grid)
    cum, meta = ops.cumulative_intersects(T(ref["nth"]), depths)
    np.testing.assert_array_equal(N(cum), ref["cum"])
    m, d_or, d_and = N(meta).tolist()[:3]
    assert m == ref["M"] and d_or == d_and == 0
    gids, bins, isect = ops.bin_and_sort_tiles(g["n"], ref["M"], xys, depths, radii, cum, tb,
                                               want_isect_ids=True)
    np.testing.assert_array_equal(N(bins), ref["bins"])
    np.testing.assert_array_equal(N(gids), ref["gids"])
    np.testing.assert_array_equal(N(isect), ref["isect_sorted"])


@pytest.mark.parametrize("grid", G.BIN_GRIDS, ids=G.BIN_IDS)
def test_bin_and_sort_gaussians_int64(cuda, grid):
    """The drop-in bin_and_sort_gaussians (map, the 8-pass int64 sort, bin
    edges into max(M, tiles) rows) and get_tile_bin_edges on the reference's
    sorted keys."""
    import gsplat
    g, ref, tb, xys, radii, depths = _grid_dev(grid)
    nt, M = g["ntiles"], ref["M"]
    isect, ids, isect_sorted, gids, bins = gsplat.bin_and_sort_gaussians(
        g["n"], M, xys, depths, radii, T(ref["cum"]), tb)
    np.testing.assert_array_equal(N(isect), ref["isect"])
    np.testing.assert_array_equal(N(ids), ref["map_ids"])
    np.testing.assert_array_equal(N(isect_sorted), ref["isect_sorted"])
    np.testing.assert_array_equal(N(gids), ref["gids"])
    assert bins.shape[0] == max(M, nt)
    np.testing.assert_array_equal(N(bins)[:nt], ref["bins"])
    assert not N(bins)[nt:].any()
    edges = gsplat.get_tile_bin_edges(M, T(ref["isect_sorted"]))
    assert edges.shape[0] == max(M, nt)  # the last tile is never empty
    np.testing.assert_array_equal(N(edges)[:nt], ref["bins"])
    assert not N(edges)[nt:].any()


def test_overflow_rebuild_respects_capacity(cuda):
    """gsvc_bin_tiles_counted with tile_cap 256 and a capacity that ends inside
    an over-full tile's segment: meta[1] reports it, nothing at or past the
    capacity is written, and every tile whose segment ends inside the capacity
    is exact.  Both id buffers are allocated at tiles * 256 and filled with a
    sentinel, so every write the kernels can make lands in memory owned here."""
    from gsvc_amd import _lib as L
    g, ref, tb, xys, radii, _ = _grid_dev((129, 65))
    nt, bins_ref, counts = g["ntiles"], ref["bins_capped"], ref["counts"]
    over = np.flatnonzero(counts > G.TILE_CAP)
    assert over.size >= 2 and over[0] < G.SCAN_CHUNK < over[-1]
    capacity = int(bins_ref[over[0], 0]) + 100  # inside the first over-full tile's 256 slots
    assert bins_ref[over[0], 0] < capacity < bins_ref[over[0], 1]
    full, sentinel = nt * G.TILE_CAP, -7
    scratch = torch.full((full,), sentinel, dtype=torch.int32, device=cuda)
    gids = torch.full((full,), sentinel, dtype=torch.int32, device=cuda)
    bins = torch.empty((nt, 2), dtype=torch.int32, device=cuda)
    meta = torch.empty((2,), dtype=torch.int32, device=cuda)
    ws = torch.empty((L.size("gsvc_bin_tiles_counted_workspace_bytes", nt) // 4 + 1,), dtype=torch.int32,
                     device=cuda)
    L.call("gsvc_bin_tiles_counted", g["n"], L.ptr(xys), L.ptr(radii), tb[0], tb[1],
           capacity, G.TILE_CAP, L.ptr(scratch), L.ptr(gids), L.ptr(bins), L.ptr(meta),
           L.ptr(ws), 4 * ws.numel(), L.stream(cuda))
    torch.cuda.synchronize()
    assert N(meta).tolist() == [ref["M"], 1]
    np.testing.assert_array_equal(N(bins), bins_ref)
    got = N(gids)
    inside = np.flatnonzero((counts > 0) & (bins_ref[:, 1] <= capacity))
    assert inside.size > 50
    end = int(bins_ref[inside, 1].max())
    np.testing.assert_array_equal(got[:end], ref["gids_capped"][:end])
    assert (got[capacity:] == sentinel).all()
    assert (N(scratch)[capacity:] == sentinel).all()


# ---------------------------------------------------------------- forward against float64
def _empty_is_zero(img_hw3, c):
    """Every pixel of an empty tile holds what the reference holds there --
    the sum of nothing, +0.0 -- bit for bit."""
    empty = G.tile_mask(c["H"], c["W"], np.flatnonzero(c["counts"] == 0))
    assert empty.any() and not c["fwd"]["out"][empty].any()
    assert not np.ascontiguousarray(img_hw3[empty]).view(np.uint32).any()


@pytest.mark.parametrize("tagged", [True, False], ids=["sync-free", "host-sized"])
@pytest.mark.parametrize("cid", G.FORWARD_IDS)
def test_rasterize_sum_against_float64(cuda, cid, tagged):
    """rasterize_gaussians_sum on the sync-free path (depths known to be zero)
    and on the host-sized sorted path (untagged depths)."""
    from gsplat.rasterize_sum import rasterize_gaussians_sum
    from gsvc_amd.utils import depths_known_zero, mark_zero_depths
    c = G.op_case(cid)
    n = c["xys"].shape[0]
    depths = torch.zeros(n, device=cuda)
    if tagged:
        mark_zero_depths(depths)
    assert depths_known_zero(depths) == tagged
    out = rasterize_gaussians_sum(T(c["xys"]), depths, T(c["radii"]), T(c["conics"]), T(c["nth"]),
                                  T(c["colors"]), T(c["opacity"]), c["H"], c["W"], 16, 16,
                                  background=torch.ones(3, device=cuda))
    out = N(out)
    err = S.image_error(out, c["fwd"]["out"], ~c["fwd"]["borderline"])
    _report(cid, "sync-free" if tagged else "host-sized", "image", err, S.BARS["image"])
    assert err <= S.BARS["image"]
    _empty_is_zero(out, c)


MODES = {"id-slabs": (Knob.FWD_MODE, 0), "record-slabs": (Knob.RECORD_SLABS, 1), "banded": (Knob.FWD_MODE, 2)}


def _frame_args(p, dev):
    return (T(p["xyz"]), T(p["chol"]), T(p["feat"]), p["H"], p["W"], T(p["bg"]))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("cid", G.FORWARD_IDS)
def test_render_frame_against_float64(cuda, cid, mode):
    """render_frame_sum (the clamped frame render from the raw parameters) over
    id slabs, record slabs and the banded kernel; the second call runs on the
    ordered projection."""
    from gsvc_amd.render import render_frame_sum
    p, r = G.grid_case(cid)
    c = G.op_case(cid)
    with knobs(MODES[mode]):
        outs = [render_frame_sum(*_frame_args(p, cuda), cholesky_bound=T(p["bound"])) for _ in range(2)]
    assert torch.equal(outs[0], outs[1])
    img = N(outs[0])[0]
    err = float(np.abs(img.astype(np.float64) - r["render"]).max())
    _report(cid, mode, "render", err, S.GRID_BARS["render"])
    assert err <= S.GRID_BARS["render"]
    _empty_is_zero(np.ascontiguousarray(img.transpose(1, 2, 0)), c)


@pytest.mark.parametrize("cid", ["grid-R2", "grid-R1"])
def test_render_frames_two_frames(cuda, cid):
    """render_frames_sum with two different frames of one size (the case and
    its point mirror: other tiles occupied), 2 x tiles workgroups in one grid:
    each output equals its single-frame render bit for bit, and the first the
    float64 reference."""
    from gsvc_amd.render import render_frame_sum, render_frames_sum
    p, r = G.grid_case(cid)
    n = p["xyz"].shape[0]
    xyz = torch.cat([T(p["xyz"]), -T(p["xyz"])])
    chol, feat = T(p["chol"]).repeat(2, 1), T(p["feat"]).repeat(2, 1)
    bound, bg = T(p["bound"]), T(p["bg"])
    both = render_frames_sum(xyz, chol, feat, [n, n], p["H"], p["W"], bg, cholesky_bound=bound)
    assert not torch.equal(both[0], both[1])
    for b in (0, 1):
        sl = slice(b * n, (b + 1) * n)
        one = render_frame_sum(xyz[sl], chol[sl], feat[sl], p["H"], p["W"], bg, cholesky_bound=bound)
        assert torch.equal(both[b], one[0]), b
    err = float(np.abs(N(both[0]).astype(np.float64) - r["render"]).max())
    _report(cid, "two-frames", "render", err, S.GRID_BARS["render"])
    assert err <= S.GRID_BARS["render"]


# ---------------------------------------------------------------- the fused step against float64
def _check_grid(cid, what, render, losses, g):
    errs = G.grid_errors(cid, N(render), N(losses) if torch.is_tensor(losses) else losses, N(g))
    flat = []
    for k in ("render", "loss_abs", "loss_rel") + tuple(n for n, _ in S.PARAM_GRADS):
        v = errs[k]
        if isinstance(v, tuple):
            whole, edge, tile, where = v
            flat += [(k + ".whole", whole, k), (k + ".edge", edge, k), (f"{k}.tile[{where}]", tile, k)]
        else:
            flat.append((k, v, k))
    for name, val, k in flat:
        _report(cid, what, name, val, S.GRID_BARS[k])
    for name, val, k in flat:
        assert val <= S.GRID_BARS[k], (cid, what, name, val, S.GRID_BARS[k])


@pytest.mark.parametrize("cid", G.STEP_IDS)
def test_fused_step_against_float64(cuda, tile_kernel, cid):
    """gsvc_train_step_sum (both tile kernels, L2 and L1): the clamped render,
    both losses and the nine gradient columns against train_grads64."""
    p, r = G.grid_case(cid)
    render, losses, g = _step(p, cuda)
    _check_grid(cid, tile_kernel, render, losses, g)


@pytest.mark.parametrize("cid", G.STEP_IDS)
def test_fused_step_deterministic(cuda, cid):
    """Deterministic mode: the same bars, and two runs bitwise equal."""
    p, r = G.grid_case(cid)
    with deterministic():
        a = _step(p, cuda)
        b = _step(p, cuda)
    _check_grid(cid, "det", *a)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_production_train_iter_r1(cuda):
    """GaussianVideoFrame.train_iter on R1 for three steps at learning rate 0
    (the bound step, carried bins, the tile kernel enqueued ahead), read as
    test_sum_edges.test_production_train_iter reads it."""
    cid = "grid-R1"
    p, r = G.grid_case(cid)
    H, W = p["H"], p["W"]
    m = _model(p, cuda, lr=0.0, fused_train=True)
    gt = T(p["gt"]).view(1, 3, H, W)
    names = ["_xyz", "_cholesky", "_features_dc"]
    start = {k: getattr(m, k).detach().clone() for k in names}
    with torch.no_grad():
        render = m()["render"][0].clone()
    for it in (1, 2, 3):
        loss, psnr = m.train_iter(gt, it)
        torch.cuda.synchronize()
        cols = [-m.optimizer.state[getattr(m, k)]["neg_pre_grad"] for k in names]
        cols.append(torch.zeros(len(p["xyz"]), 1, device=cuda))
        mse = 10.0 ** (-psnr / 10.0)
        assert math.isclose(mse, float(loss), rel_tol=1e-12)
        _check_grid(cid, f"train_iter-{it}", render, np.array([float(loss), r["losses"][1]]),
                    torch.cat(cols, 1))
        for k in names:
            assert torch.equal(getattr(m, k).detach(), start[k]), (it, k)
    assert m.fused_steps == 3
    assert m._bound_step.tiled_steps >= 1
