"""Premises of tests/alpha_cases.py, no GPU: each scripted case has the per-tile
counts and the path property it exists for; the C oracle (the float32
restatement) agrees with the float64 references outside the borderline mask
within a quarter of the kernels' bars; the borderline mask stays small (a
condition on the seeds); and the two float64 gradient references -- autograd of
the forward, and the statement of backward.cu's recursion -- agree wherever the
0.99 clamp is out of play, which ties the recursion to a true derivative."""
import numpy as np
import pytest

import alpha_cases as A


def _tile_pixels(c, t):
    for tt, ii, jj, r0, r1 in A._tiles(c):
        if tt == t:
            return ii, jj, r0, r1
    raise KeyError(t)


@pytest.mark.parametrize("cid", [i for i in A.F64_IDS if i.startswith("shape-")])
def test_shape_cases_reach_the_edges(cid):
    c = A.BY_ID[cid]
    H, W = (int(v) for v in cid[6:].split("x"))
    assert (c["H"], c["W"]) == (H, W)
    listed = np.unique(np.concatenate([c["gids"][a:b] for a, b in c["bins"]]))
    x, y = c["xys"][listed, 0], c["xys"][listed, 1]
    outside = (x > W - 0.5) | (y > H - 0.5)
    inside = (x > -0.5) & (x < W - 0.5) & (y > -0.5) & (y < H - 0.5)
    r = c["radii"][listed]
    straddle = inside & ((x + r > W - 0.5) | (y + r > H - 0.5))
    assert outside.any() and straddle.any()
    assert A.reference(cid)["fwd"]["blend"][-1].any()  # the last (edge) tile blends something


def test_shape_set():
    got = {(c["H"], c["W"]) for c in A.CASES if c["id"].startswith("shape-")}
    assert got == {(1, 1), (1, 37), (37, 1), (5, 3), (15, 17), (17, 15), (33, 18), (20, 70), (37, 45)}
    assert A.BY_ID["shape-33x18"]["W"] % 4 == 2 and A.BY_ID["shape-20x70"]["W"] % 16 == 6


@pytest.mark.parametrize("cid", ["counts-faint", "counts-opaque"])
def test_count_cases(cid):
    c = A.BY_ID[cid]
    assert list(c["counts"]) == A.COUNTS
    for n in (0, 1, 24, 25, 64, 65, 88, 89, 128, 129, 257, 7, 8, 9, 63):
        assert n in A.COUNTS
    # an empty tile next to a full one
    assert A.COUNTS[0] == 257 and A.COUNTS[1] == 0 and A.COUNTS[15:17] == [0, 257]
    fwd = A.reference(cid)["fwd"]
    if cid.endswith("faint"):
        assert not fwd["stopped"].any() and fwd["T"].min() > 10 * A.T_STOP
    else:
        assert fwd["stopped"].mean() > 0.3
        # stops on both sides of the first chunk in the dense tiles
        ii, jj, r0, r1 = _tile_pixels(c, 0)
        sp = fwd["stop_pos"][ii, jj]
        assert ((sp >= 0) & (sp < 64)).any() and (sp >= 64).any()
    # every populated tile blends something; the dense tiles reach past entry 64
    for t, B in enumerate(fwd["blend"]):
        assert B.any() == (A.COUNTS[t] > 0) or A.COUNTS[t] < 8
    assert fwd["blend"][0][:, 64:].any()


@pytest.mark.parametrize("count", [65, 89, 129, 257])
def test_allstop_cases(count):
    c = A.BY_ID[f"allstop-{count}"]
    fwd = A.reference(c["id"])["fwd"]
    assert list(c["counts"]) == [30, count, 30, count]
    # tile 1: all but one pixel stop inside the first chunk; the last one goes on
    t, (pi, pj) = c["claims"]["approached"]
    ii, jj, r0, r1 = _tile_pixels(c, t)
    live = (ii == pi) & (jj == pj)
    assert live.sum() == 1 and ii.size == 64
    assert fwd["stopped"][ii, jj][~live].all() and (fwd["stop_pos"][ii, jj][~live] < 64).all()
    assert not fwd["stopped"][pi, pj] and fwd["idx"][pi, pj] >= r0 + 64
    # tile 3: every pixel stops inside the first chunk, the list goes on
    ii, jj, r0, r1 = _tile_pixels(c, c["claims"]["taken"])
    sp = fwd["stop_pos"][ii, jj]
    assert fwd["stopped"][ii, jj].all() and sp.max() < 48 and r1 - r0 == count > 64
    assert fwd["idx"][ii, jj].max() < r0 + 48  # the backward's kend cuts every later chunk


def test_blockedge_distances():
    c = A.BY_ID["blockedge"]
    fwd = A.reference("blockedge")["fwd"]
    ii, jj, r0, r1 = _tile_pixels(c, 4)
    assert r1 - r0 == 40 > 24 and (ii.min(), jj.min()) == (16, 16)  # grouped lists
    ids = list(c["gids"][r0:r1])
    seen = set()
    for e in c["claims"]["edges"]:
        g = e["id"]
        ext = A.ellipse_extent(c["conics"][g], c["opacity"][g, 0])[e["axis"]]
        centre = float(c["xys"][g, e["axis"]])
        end = centre + e["side"] * ext
        d = e["side"] * (end - e["line"])  # > 0: the end is past the line, the line's pixels inside
        assert abs(d) <= 0.05 and (d > 0) == e["inside"], (e, d)
        assert abs(abs(d) - 0.04) < 1e-3
        assert e["line"] % 4 == (0 if e["side"] > 0 else 3) and 16 <= e["line"] < 32
        # the pixel on the line takes the entry exactly when the end is past it,
        # and it is not borderline
        pi, pj = (e["other"], e["line"]) if e["axis"] == 0 else (e["line"], e["other"])
        p = np.flatnonzero((ii == pi) & (jj == pj))[0]
        assert fwd["blend"][4][p, ids.index(g)] == e["inside"]
        assert not fwd["borderline"][pi, pj]
        seen.add((e["axis"], e["side"], e["inside"]))
    assert len(seen) == 8 and len(c["claims"]["edges"]) == 16


def test_noblend_nine_tiles_opacities_clamp():
    c = A.BY_ID["noblend"]
    fwd = A.reference("noblend")["fwd"]
    for t in c["claims"]["noblend"]:
        ii, jj, r0, r1 = _tile_pixels(c, t)
        assert r1 - r0 == 30 and not fwd["blend"][t].any() and (fwd["idx"][ii, jj] == 0).all()
        assert (r0 == 0) == (t == 0)
    c = A.BY_ID["nine-tiles"]
    fwd = A.reference("nine-tiles")["fwd"]
    assert len(c["bins"]) == 9
    for t, (r0, r1) in enumerate(c["bins"]):
        assert c["gids"][r0] == 0 and fwd["blend"][t][:, 0].any()
    c = A.BY_ID["opacities"]
    fwd = A.reference("opacities")["fwd"]
    assert (c["counts"] > 24).any() and (c["counts"] <= 24).any()
    blended = np.zeros(c["xys"].shape[0], bool)
    for (r0, r1), B in zip(c["bins"], fwd["blend"]):
        blended[c["gids"][r0:r1][B.any(0)]] = True
    k = np.arange(c["xys"].shape[0]) % len(A.OPACITIES)
    assert not blended[k < 2].any() and not blended[(k == 4) | (k == 5)].any()
    assert blended[k == 6].any() and blended[k == 2].any() and blended[k == 3].any()
    lg = np.log(255.0 * np.array(A.OPACITIES[4:7]))
    assert lg[0] < -0.01 < lg[1] < 0 < lg[2]
    fwd = A.reference("clamp-99")["fwd"]
    assert fwd["hi99"].sum() >= 10
    for cid in A.F64_IDS:
        if cid not in ("clamp-99", "opacities"):
            assert not A.reference(cid)["fwd"]["hi99"].any(), cid


def test_caller_cases():
    c = A.BY_ID["caller-nonpd"]
    a, b, cc = (float(v) for v in c["conics"][0])
    assert a * cc - b * b < 0
    ii, jj = np.mgrid[0:c["H"], 0:c["W"]]
    _, _, s = A._sigma(c["xys"].astype(np.float64), c["conics"].astype(np.float64), 0, ii, jj)
    assert (s < -0.1).any() and (s > 0.1).any()
    c = A.BY_ID["caller-needle"]
    a, b, cc = (float(v) for v in c["conics"][0])
    assert 0 < a * cc - b * b < a * cc / 8192.0
    assert np.isnan(A.BY_ID["caller-nancolor"]["colors"]).sum() == 1
    for cid in A.CALLER_IDS:
        c = A.BY_ID[cid]
        assert all(c["gids"][r0] == 0 for r0, r1 in c["bins"])


@pytest.mark.parametrize("cid", A.F64_IDS)
def test_borderline_cap(cid):
    """At most 2 % of the pixels are borderline, and every tile keeps a pixel
    that is not: a condition on the case's inputs."""
    c = A.BY_ID[cid]
    bd = A.reference(cid)["fwd"]["borderline"]
    assert bd.mean() <= 0.02
    for t, ii, jj, r0, r1 in A._tiles(c):
        assert not bd[ii, jj].all()


@pytest.mark.parametrize("cid", A.F64_IDS)
def test_oracle_against_float64(cid, oracle):
    """The float32 restatement against float64 outside the borderline mask:
    final_idx equal, image, T and the gradients within a quarter of the bars."""
    c = A.BY_ID[cid]
    r = A.reference(cid)
    fwd, keep = r["fwd"], ~r["fwd"]["borderline"]
    out, Ts, idx, g = A.oracle_run(c, r["v_out"], r["v_alpha"])
    np.testing.assert_array_equal(idx[keep], fwd["idx"][keep])
    assert np.abs(out - fwd["out"])[keep].max() <= A.BARS["image"] / 4
    assert np.abs(Ts - fwd["T"])[keep].max() <= A.BARS["T"] / 4
    for name, (whole, edge) in A.grad_errors(c, g, r["rec"]).items():
        assert max(whole, edge) <= A.BARS[name] / 4, (name, whole, edge)


@pytest.mark.parametrize("cid", A.F64_IDS)
def test_gradient_references_agree(cid):
    """Autograd of the float64 forward (decisions fixed, cross term halved)
    equals the recursion to 1e-10 of each tensor's largest element wherever the
    0.99 mask is empty."""
    c = A.BY_ID[cid]
    r = A.reference(cid)
    if r["fwd"]["hi99"].any():
        assert cid in ("clamp-99", "opacities")
        return
    ag = A.alpha_backward64_autograd(c, r["fwd"], r["v_out"], r["v_alpha"])
    for name in A.GRADS:
        assert A.rel_error(ag[name], r["rec"][name]) <= 1e-10, name


@pytest.mark.parametrize("cid,kind", A.VARIANT_IDS)
def test_oracle_variants(cid, kind, oracle):
    """v_out alone, v_out_alpha alone, and a caller-lowered final_idx (10 % of
    the pixels): the restatement against the recursion."""
    c = A.BY_ID[cid]
    fwd = A.reference(cid)["fwd"]
    vo, va, fi, ref = A.variant(cid, kind)
    if kind == "lowered":
        assert 0.03 < (fi != fwd["idx"]).mean() <= 0.12 and (fi <= fwd["idx"]).all()
    else:
        assert not (va if kind == "out" else vo).any()
    g = A.oracle_run(c, vo, va, fi)[3]
    for name, (whole, edge) in A.grad_errors(c, g, ref).items():
        assert max(whole, edge) <= A.BARS[name] / 4, (name, whole, edge)
