"""Premises of tests/grid_cases.py, no GPU: the integer binning reference
equals the C oracle on every binning grid; each grid reaches the sort width and
scan trips it exists for, with the placed tiles non-empty and different from
their neighbours across every chunk join; the rendered grids have the occupied
tiles they claim and no borderline decision; a single tile pair's share of
either loss on the 8385-tile frame is at least twice the loss bar, so a dropped
or doubled pair cannot hide inside it; and both float32 restatements are inside
the figures the grid bars are four times of."""
import numpy as np
import pytest

import grid_cases as G
import sum_cases as S

FUSED_KEYS = ("render", "loss_abs", "loss_rel") + tuple(n for n, _ in S.PARAM_GRADS)


# ---------------------------------------------------------------- binning grids
@pytest.mark.parametrize("grid", G.BIN_GRIDS, ids=G.BIN_IDS)
def test_binning_reference_equals_oracle(grid, oracle):
    g = G.bin_grid(*grid)
    ref = g["ref"]
    tb = (g["tbx"], g["tby"], 1)
    m, cum = oracle.cumulative_intersects(ref["nth"])
    assert m == ref["M"]
    np.testing.assert_array_equal(cum, ref["cum"])
    isect, gids = oracle.map_intersects(g["xys"], g["depths"], g["radii"], cum, tb, m)
    np.testing.assert_array_equal(isect, ref["isect"])
    np.testing.assert_array_equal(gids, ref["map_ids"])
    isect_sorted, gids_sorted = oracle.sort_pairs(isect, gids)
    np.testing.assert_array_equal(isect_sorted, ref["isect_sorted"])
    np.testing.assert_array_equal(gids_sorted, ref["gids"])
    bins = oracle.tile_bin_edges(isect_sorted, g["ntiles"])
    np.testing.assert_array_equal(bins, ref["bins"])
    _, _, s2, g2, b2 = oracle.bin_and_sort(g["xys"], g["depths"], g["radii"], cum, tb, m)
    np.testing.assert_array_equal(g2, ref["gids"])
    np.testing.assert_array_equal(b2[:g["ntiles"]], ref["bins"])
    assert not b2[g["ntiles"]:].any()


@pytest.mark.parametrize("grid", G.BIN_GRIDS, ids=G.BIN_IDS)
def test_binning_grid_claims(grid):
    g = G.bin_grid(*grid)
    ref, nt, tbx, tby = g["ref"], g["ntiles"], g["tbx"], g["tby"]
    counts = ref["counts"]
    assert nt == tbx * tby and G.bits_for(nt) == G.SORT_BITS[nt]
    assert 2200 <= g["n"] <= 3400
    # exact centres, every radius class, centres off every side
    assert (g["xys"].astype(np.float64) * G.SUB == g["cxy"]).all()
    box, r = ref["box"], g["radii"]
    area = np.where(r > 0, (box[:, 1] - box[:, 0]) * (box[:, 3] - box[:, 2]), 0)
    np.testing.assert_array_equal(area, ref["nth"])
    assert (r == 0).sum() >= 200 and (area == 1).sum() >= 1300
    if tbx >= 3 and tby >= 3:  # (a 3 x 3 box is clipped on the grid's border rows and columns)
        assert (area == 9).sum() >= (300 if min(tbx, tby) >= 16 else 100)
    assert (area >= min(nt, max(tbx, tby))).sum() >= 2  # the whole long side of the grid
    cx, cy = g["cxy"][:, 0], g["cxy"][:, 1]
    for off in (cx < 0, cx >= tbx * G.UNIT, cy < 0, cy >= tby * G.UNIT):
        assert off.sum() >= 40 and (off & (area > 0)).any() and (off & (area == 0) & (r > 0)).any()
    # ids are not in tile order
    first = np.full(g["n"], -1)
    first[ref["map_ids"][::-1]] = ref["map_tiles"][::-1]
    assert (np.diff(first[first >= 0]) < 0).sum() > 500 or nt <= 2
    # tile 0, the last tile and both tiles of every join: non-empty, unlike their neighbours
    assert counts[0] > 0 and counts[-1] > 0
    if nt > 2:
        assert counts[0] != counts[1] and counts[-1] != counts[-2]
    js = G.joins(nt)
    assert len(js) == (nt - 1) // G.SCAN_CHUNK
    for j in js:
        assert counts[j - 1] > 0 and counts[j] > 0 and counts[j - 1] != counts[j], j
        assert counts[j - 2] != counts[j - 1], j
        if j + 1 < nt:
            assert counts[j] != counts[j + 1], j
    # the capped scan and the uncapped total diverge: a tile past 256 before the
    # first join, and after it one above 64 and one above 256
    if nt > 2:
        assert (counts[:G.SCAN_CHUNK] > G.TILE_CAP).any()
        assert ref["M_capped"] < ref["M"]
    if js:
        after = counts[G.SCAN_CHUNK:]
        assert (after > 64).any() and (after > G.TILE_CAP).any()
        if nt >= G.SCAN_CHUNK + 8:
            assert ((after > 64) & (after <= G.TILE_CAP)).any()
        # a non-empty tile after the over-full one: its capped start differs from its uncapped one
        later = np.flatnonzero(counts > 0)
        later = later[later > G.SCAN_CHUNK + np.flatnonzero(after > G.TILE_CAP)[0]]
        if later.size:
            assert (ref["bins"][later, 0] != ref["bins_capped"][later, 0]).all()
    for t, k in g["placed"].items():
        assert counts[t] >= k
    # the reference's own consistency
    assert counts.sum() == ref["M"] == ref["gids"].size == int(ref["cum"][-1])
    assert ref["gids_capped"].size == ref["M_capped"] == int(ref["bins_capped"][:, 1].max())
    for t in {0, nt - 1, *js, *[j - 1 for j in js]}:
        ids = ref["gids"][slice(*ref["bins"][t])]
        assert ids.size == counts[t] and (np.diff(ids) > 0).all()


def test_binning_grids_cover_the_thresholds():
    tiles = [x * y for x, y in G.BIN_GRIDS]
    assert sorted({G.bits_for(t) for t in tiles}) == [0, 1, 8, 9, 13, 14, 15, 16, 17]
    trips = sorted({-(-t // G.SCAN_CHUNK) for t in tiles})
    assert trips == [1, 2, 3, 8, 9]
    assert G.SCAN_CHUNK in tiles and G.SCAN_CHUNK + 1 in tiles
    assert any(t % 2 and t > G.SCAN_CHUNK for t in tiles)
    # three sort passes (more than 16 bits) only on the last grid
    assert [t for t in tiles if G.bits_for(t) > 16] == [65792]


# ---------------------------------------------------------------- rendered grids
def test_rendered_grid_sizes():
    for name, tiles, m8, m128 in (("R2", 525, 5, 13), ("R1", 8385, 1, 65), ("R3", 16512, 0, 0)):
        H, W, tbx, tby = G.grid_dims(name)
        assert tbx * tby == tiles and tiles % 8 == m8 and tiles % 128 == m128
    # R2 is whole tiles on both axes (400 = 25 x 16, 336 = 21 x 16): it is there for its tile
    # count; the partial right and bottom tiles come with R1 (11 columns, 7 rows) and R3
    H, W, tbx, tby = G.grid_dims("R2")
    assert (W % 16, H % 16) == (0, 0)
    H, W, tbx, tby = G.grid_dims("R1")
    assert (tbx, tby, W - 16 * (tbx - 1), H - 16 * (tby - 1)) == (129, 65, 11, 7)
    # the second publish_loss trip of R1: 96 pairs and the odd tail
    assert 8385 // 2 - G.LOSS_TRIP // 2 == 96 and 8385 % 2 == 1
    # two frames of R2 / R1 in one launch move the run tail again
    assert (2 * 525) % 128 == 26 and (2 * 8385) % 128 == 2 and 2 * 8385 == 16770
    H, W, tbx, tby = G.grid_dims("R3")
    assert (tbx, tby) == (129, 128) and W % 16 == 11 and H % 16 == 8


@pytest.mark.parametrize("cid", G.GRID_IDS)
def test_rendered_grid_claims(cid):
    p, r = G.grid_case(cid)
    name = p["claims"]["grid"]
    H, W, tbx, tby = G.grid_dims(name)
    nt = tbx * tby
    c, pr = r["c"], r["proj"]
    assert (p["H"], p["W"]) == (H, W) and len(c["bins"]) == nt
    placed = p["claims"]["placed"]
    assert len(placed) == G.OCCUPIED and set(G.required_tiles(name)) <= set(placed)
    for t in (0, nt - 1) + ((8190, 8191, 8192, 8193) if nt > 8193 else ()):
        assert t in placed
    tail = (nt // 128) * 128
    assert sum(t >= tail for t in placed) >= (4 if nt % 128 else 0)  # (R3 is whole runs: no tail)
    assert {placed[t] for t in placed} == set(G.K_CYCLE)
    if nt > 8193:
        assert len({placed[t] for t in (8190, 8191, 8192, 8193)}) == 4
    # the placed splats list the tile they were placed in, and nearly all that tile alone
    # (the builder's moves, up to a pixel each on a frame this wide, carry a few over a
    # tile line); ids shuffled
    tile_of = p["claims"]["tile_of"]
    small = tile_of >= 0
    box = pr["box"]
    area = (box[:, 1] - box[:, 0]) * (box[:, 3] - box[:, 2])
    tx, ty = tile_of % tbx, tile_of // tbx
    inside = (box[:, 0] <= tx) & (tx < box[:, 1]) & (box[:, 2] <= ty) & (ty < box[:, 3])
    assert inside[small].all() and (area[small] == 1).mean() >= 0.97 and (area[small] <= 4).all()
    assert (np.diff(tile_of[small]) < 0).sum() > 300
    # the larger ones cross tile joins and reach the right and bottom edges
    big = ~small
    assert big.sum() == G.N_LARGE and (area[big] >= 2).all() and (area[big] >= 6).sum() >= 6
    assert (box[big, 1] == tbx).sum() >= 4 and (box[big, 3] == tby).sum() >= 4
    # counts: a placed tile holds its k and whatever larger splats cross it; every other
    # listed tile only larger splats; everything else is empty
    counts = c["counts"]
    spill = int((area[small] > 1).sum())
    for t, k in placed.items():
        assert k <= counts[t] <= k + G.N_LARGE + spill
    others = np.setdiff1d(np.flatnonzero(counts), list(placed))
    assert (counts[others] <= G.N_LARGE + spill).all()
    assert (counts == 0).sum() >= nt - G.OCCUPIED - 40 * G.N_LARGE - 3 * spill
    assert counts[0] > 0 and counts[-1] > 0
    assert p["loss"] == ("L1" if cid.endswith("L1") else "L2")
    assert (p["bg"] == 1).all() and not p["rgbw_train"]


@pytest.mark.parametrize("cid", G.GRID_IDS)
def test_rendered_grids_have_no_borderline_decision(cid):
    p, r = G.grid_case(cid)
    for k, floor in S.MARGIN_FLOOR.items():
        assert r["margins"][k] >= floor, (k, r["margins"][k])
    assert not r["fwd"]["border_pairs"] and not r["fwd"]["borderline"].any()
    # (the builder cleared the tile boxes beforehand; what the loop moved is a handful)
    assert p["nudged"] <= 32


@pytest.mark.parametrize("cid", G.FORWARD_IDS)
def test_op_view_of_rendered_grids(cid):
    """The float32 projection decides every radius and tile box as float64
    does, so the float64 lists are the operator's; its borderline mask stays
    inside the cap."""
    p, r = G.grid_case(cid)
    c = G.op_case(cid)
    np.testing.assert_array_equal(c["radii"], r["proj"]["radius"])
    np.testing.assert_array_equal(c["box"], r["proj"]["box"])
    assert int(c["nth"].sum()) == r["M"] == c["gids"].size
    assert c["fwd"]["borderline"].mean() <= S.MASK_CAP
    empty = G.tile_mask(c["H"], c["W"], np.flatnonzero(c["counts"] == 0))
    assert empty.mean() > 0.75 and not c["fwd"]["out"][empty].any()  # an empty tile sums nothing: 0.0


def test_loss_sensitivity():
    """On R1 the smallest share of either loss that one tile pair (or the odd
    last tile, 11 x 7 pixels) contributes is at least twice the relative loss
    bar: a pair dropped or added twice by the loss workgroup's second trip or
    its tail cannot pass."""
    for cid in ("grid-R1", "grid-R1-L1"):
        s2, s1 = G.loss_sensitivity(cid)
        print(f"GRID-LOSS {cid} smallest pair share mse {s2:.3e} l1 {s1:.3e} "
              f"bar {S.GRID_BARS['loss_rel']:.3e}")
        assert min(s2, s1) >= 2.0 * S.GRID_BARS["loss_rel"]
    assert S.GRID_BARS["loss_rel"] == S.BARS["loss_rel"] and S.GRID_BARS["loss_abs"] == S.BARS["loss_abs"]


def test_grid_bars_are_four_times_worst():
    assert set(S.GRID_BARS) == set(S.BARS)
    for k, v in S.BARS.items():
        assert S.GRID_BARS[k] == 4.0 * max(S.WORST[k], S.WORST_GRID.get(k, 0.0)) >= v
    assert S.GRID_BARS["image"] == S.BARS["image"]


@pytest.mark.parametrize("cid", G.GRID_IDS)
def test_grid_restatements_inside_worst(cid, oracle):
    """As test_sum_cases_cpu.test_fused_restatements_inside_worst, with the
    grid table and publish_loss's summation for the float32 losses."""
    p, r = G.grid_case(cid)
    worst = {k: max(S.WORST[k], S.WORST_GRID.get(k, 0.0)) for k in S.WORST}
    for run, room in ((S.oracle_fused, 1.25), (G.float32_fused, 2.0)):
        e = G.grid_errors(cid, *run(p))
        for k in FUSED_KEYS:
            if cid in G.STEP_IDS or k == "render":
                assert S.worst_of(e, k) <= room * worst[k], (run.__name__, k, e[k])
    if cid in G.FORWARD_IDS:
        c = G.op_case(cid)
        keep = ~c["fwd"]["borderline"]
        for run, room in ((S.oracle_op_forward, 1.25), (S.float32_op_forward, 2.0)):
            out, idx = run(c)
            assert (idx[keep] == c["fwd"]["idx"][keep]).all()
            assert S.image_error(out, c["fwd"]["out"], keep) <= room * S.WORST["image"]
