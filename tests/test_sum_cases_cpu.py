"""Premises of tests/sum_cases.py, no GPU: the two statements of every gradient
(the formulas written out, and torch autograd of the float64 forward with the
decisions fixed) agree; each scripted case has the per-tile counts, rectangle
properties and pass-through shares it exists for; no gradient case has a
decision within its margin and the op-level image mask stays within its cap (a
condition on the cases, not a measurement); and both float32 restatements --
the C oracle and the sequential float32 chain -- are inside the figures the
bars are four times of."""
import numpy as np
import pytest

import sum_cases as S

FUSED_KEYS = ("render", "loss_abs", "loss_rel") + tuple(n for n, _ in S.PARAM_GRADS)


# ---------------------------------------------------------------- the two statements
@pytest.mark.parametrize("cid", S.FUSED_IDS)
def test_fused_gradient_statements_agree(cid):
    """chain_np (backward.cu / backward2d.cu written out) against autograd from
    the raw parameters, quirks applied: 1e-10 of each tensor's largest element;
    the renders and the loss to 1e-12."""
    p, r = S.fused_case(cid)
    img, loss, g = S.train_grads64_autograd(p, r)
    if r["M"] >= 1:
        assert np.abs(img - r["render"]).max() <= 1e-12
        assert abs(loss - r["losses"][1 if p["loss"] == "L1" else 0]) <= 1e-12
    for name, sl in S.PARAM_GRADS:
        assert S.rel_error(g[:, sl], r["grads"][:, sl]) <= 1e-10, name
        if name != "d_rgb_W" or p["rgbw_train"]:
            assert (r["M"] < 1) == (not r["grads"][:, sl].any()), name


@pytest.mark.parametrize("cid", S.OP_IDS)
def test_op_gradient_statements_agree(cid):
    c = S.op_case(cid)
    fwd, ref = S.op_reference(cid)
    formula = S.sum_backward64_formula(c, fwd, c["v_out"])
    for name in S.OP_GRADS:
        assert S.rel_error(formula[name], ref[name]) <= 1e-10, name
    # an entry after a pixel's final_idx is not kept, and only the first 256 are
    for T, (r0, r1) in zip(fwd["tiles"], c["bins"]):
        assert T["g"].size == min(r1 - r0, S.TILE_PIX)
        if T["keep"].any():
            ii, jj = T["ii"], T["jj"]
            pos = r0 + np.arange(T["g"].size)
            assert not (T["keep"] & (pos[None, :] > fwd["idx"][ii, jj][:, None])).any()


# ---------------------------------------------------------------- no borderline decisions
@pytest.mark.parametrize("cid", S.FUSED_IDS)
def test_fused_cases_have_no_borderline_decision(cid):
    p, r = S.fused_case(cid)
    for k, floor in S.MARGIN_FLOOR.items():
        assert r["margins"][k] >= floor, (k, r["margins"][k])
    if r["fwd"] is not None:
        assert not r["fwd"]["border_pairs"] and not r["fwd"]["borderline"].any()
    assert p["nudged"] <= 16  # the builder moved a handful of splats, not the case


@pytest.mark.parametrize("cid", S.OP_IDS)
def test_op_cases_mask_and_gradients(cid):
    """After the builder's nudges no pair of an op-level case is borderline, so
    the gradients carry no decision within its margin and the image mask (cap
    0.03 % of the pixels) is empty."""
    c = S.op_case(cid)
    fwd = c["fwd"]
    assert fwd["borderline"].mean() <= S.MASK_CAP
    assert not fwd["border_pairs"] and c["nudged"] <= 8
    src = S.A.BY_ID.get(cid)
    if src is not None:  # the geometry is alpha_cases', moved by at most two nudges
        assert np.abs(c["xys"] - src["xys"]).max() <= 2.01 * np.abs(S.NUDGE).max()
        assert c["gids"] is src["gids"] and c["conics"] is src["conics"]


# ---------------------------------------------------------------- claims of the cases
def _tile_stats(r):
    """Per tile: entries, in-image pixels, pass-through share of them, kept
    pairs per entry."""
    out = []
    for T in r["fwd"]["tiles"]:
        ok = r["passes"][T["ii"], T["jj"]].all(1)
        k = T["g"].size
        out.append((k, T["ii"].size, ok.mean(), T["keep"].sum() / max(k, 1)))
    return out


@pytest.mark.parametrize("cid", S.FUSED_COUNT_IDS)
def test_counts_case(cid):
    p, r = S.fused_case(cid)
    c, pr = r["c"], r["proj"]
    assert (p["H"], p["W"]) == (58, 74) and len(c["bins"]) == 20
    assert list(c["counts"]) == S.COUNTS
    for n in (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300):
        assert n in S.COUNTS
    # one tile per splat, radius 3 or 4, ids not in tile order
    box = pr["box"]
    assert ((box[:, 1] - box[:, 0]) * (box[:, 3] - box[:, 2]) == 1).all()
    assert set(np.unique(pr["radius"])) == {3, 4} and (pr["radius"] == 4).mean() > 0.2
    tile_of = box[:, 2] * 5 + box[:, 0]
    np.testing.assert_array_equal(tile_of, p["claims"]["tile_of"])
    assert (np.diff(tile_of) < 0).sum() > 500
    L = r["L"]
    assert (L[:, [0, 2]] >= 0.549).all() and (L[:, [0, 2]] <= 0.951).all()
    assert (np.abs(L[:, 1]) <= 0.301).all()
    # bottom tiles hold 10 rows, right tiles 10 columns; every non-empty tile
    # passes the clamp on >= 50 % of its pixels and keeps >= 8 pairs per entry
    stats = _tile_stats(r)
    assert stats[19][1] == 100 and stats[4][1] == 160 and stats[16][1] == 160
    for t, (k, px, share, kept) in enumerate(stats):
        if k:
            assert share >= 0.5 and kept >= 8.0, (t, k, share, kept)
    out = r["out"][r["fwd"]["covered"]]
    assert (out > 1).any() and (out < 0).any() and r["passes"].mean() >= 0.93
    # the entries past 256 are not kept and their splats get exactly nothing
    dead = S.only_past_256(c)
    assert dead.sum() == (257 - 256) * 2 + (300 - 256) and not r["grads"][dead].any()
    if cid == "counts-rgbw":
        assert p["rgbw_train"] and r["grads"][:, 8].any() and np.ptp(p["rgbw"]) > 0.5
    else:
        assert not p["rgbw_train"] and (p["rgbw"] == 1).all()
    assert p["loss"] == ("L1" if cid.endswith("L1") else "L2")


def _items(rect, band):
    """Work items (rectangle rows inside the band) and their length per entry."""
    y_lo, y_hi = 8 * band, 8 * band + 7
    some = rect[:, 0] <= rect[:, 1]
    rows = np.minimum(rect[:, 3], y_hi) - np.maximum(rect[:, 2], y_lo) + 1
    items = np.where(some & (rows > 0), rows, 0)
    return items, np.where(items > 0, rect[:, 1] - rect[:, 0] + 1, 0)


@pytest.mark.parametrize("cid", ["span", "span-L1"])
def test_span_case(cid):
    """The float64 rectangles (rows.h ellipse_rect) of the span case reach every
    edge of the backward's rounds: an entry in both 8-row bands; all four
    length classes (9+, 7-8, 5-6, <= 4) in one chunk of 64; a (tile, chunk,
    band) with more than 64 work items, where an entry's run straddles a round
    and another a 16-lane row; rectangles cut by the right and bottom edges."""
    p, r = S.fused_case(cid)
    c, pr = r["c"], r["proj"]
    assert p["xyz"].shape[0] == sum(S.COUNTS) + 40 and (pr["radius"] > 8).sum() >= 30
    tbx = 5
    both = classes4 = rounds = straddle_round = straddle_row = cut_right = cut_bottom = False
    for t, (r0, r1) in enumerate(c["bins"]):
        ty, tx = divmod(t, tbx)
        ids = c["gids"][r0:min(r1, r0 + S.TILE_PIX)]
        rect = S.rect64(pr["xy"][ids], pr["conic"][ids], 16.0 * tx, 16.0 * ty)
        some = rect[:, 0] <= rect[:, 1]
        both |= bool((some & (rect[:, 2] <= 7) & (rect[:, 3] >= 8)).any())
        cut_right |= bool((some & (16 * tx + rect[:, 1] > p["W"] - 1)).any())
        cut_bottom |= bool((some & (16 * ty + rect[:, 3] > p["H"] - 1)).any())
        for c0 in range(0, len(ids), 64):
            for band in (0, 1):
                items, ilen = _items(rect[c0:c0 + 64], band)
                cls = np.where(ilen >= 9, 3, np.where(ilen >= 7, 2, np.where(ilen >= 5, 1, 0)))
                classes4 |= set(cls[items > 0]) == {0, 1, 2, 3}
                order = np.argsort(-cls, kind="stable")  # longest class first, entry order within
                off = np.cumsum(items[order]) - items[order]
                end = off + items[order]
                live = items[order] > 0
                rounds |= bool(end.max(initial=0) > 64)
                straddle_round |= bool((live & (off // 64 != (end - 1) // 64)).any())
                one_round = off // 64 == (end - 1) // 64
                straddle_row |= bool((live & one_round & (off // 16 != (end - 1) // 16)).any())
    assert both and classes4 and rounds and straddle_round and straddle_row and cut_right and cut_bottom


def test_shape_and_window_and_saturated_and_empty_cases():
    got = {(S.fused_case(i)[0]["H"], S.fused_case(i)[0]["W"]) for i in S.FUSED_IDS if i.startswith("shape-")}
    assert got == set(S.SHAPES)
    for h, w in S.SHAPES:
        p, r = S.fused_case(f"shape-{h}x{w}")
        assert r["M"] >= 1 and r["fwd"]["tiles"][-1]["keep"].any()  # the last (edge) tile blends
    # id-window: 130 entries over three 16384-id windows, 70 inside one, the rest skipped
    p, r = S.fused_case("id-window")
    c = r["c"]
    assert p["xyz"].shape[0] == 40001 and (p["H"], p["W"]) == (64, 64)
    a, b = (c["gids"][slice(*c["bins"][t])] for t in p["claims"]["tiles"])
    assert a.size == 130 and a[0] == 5 and a[-1] == 40000 and set(a // 16384) == {0, 1, 2}
    assert b.size == 70 and len(set(b // 16384)) == 1
    assert r["M"] == 200 and r["proj"]["ok"].sum() == 200
    assert (p["chol"][~r["proj"]["ok"]] == -S.BOUND).all()
    assert (np.diff(a) > 0).all() and (np.diff(b) > 0).all()
    # saturated: tanh is exactly +-1 at |xyz| = 20; centres on x = 0 / W, y = 0 / H
    p, r = S.fused_case("saturated")
    assert (p["H"], p["W"]) == (64, 48)
    sat = p["claims"]["saturated"]
    m32 = np.tanh(p["xyz"][sat])
    assert (np.abs(m32[np.abs(p["xyz"][sat]) == 20]) == 1).all()
    xy = r["proj"]["xy"][sat]
    for v in ((0, 0.0), (0, 48.0), (1, 0.0), (1, 64.0)):
        assert (np.abs(xy[:, v[0]] - v[1]) < 1e-5).any(), v
    half = r["proj"]["xy"][p["claims"]["last_half"]]
    assert ((half[:8, 0] > 47.5) & (half[:8, 0] < 48)).all()
    assert ((half[8:, 1] > 63.5) & (half[8:, 1] < 64)).all()
    listed = S.listed(r["c"])
    assert listed[sat].sum() >= 8 and listed[p["claims"]["last_half"]].all()
    rows = S.saturated_rows(p)
    assert not rows[sat].any() and rows.sum() >= 140
    assert (r["c"]["counts"] > 0).all()
    # empty: every splat skipped, a background outside [0, 1]
    p, r = S.fused_case("empty")
    assert r["M"] == 0 and not r["proj"]["ok"].any() and not r["grads"].any()
    np.testing.assert_array_equal(r["render"][:, 0, 0], [0.25, 1.0, 0.0])
    assert p["bg"].max() > 1 and p["bg"].min() < 0


def test_sum_counts_case():
    c = S.op_case("counts-sum")
    assert list(c["counts"]) == S.SUM_COUNTS and (c["H"], c["W"]) == (50, 70)
    for n in (0, 1, 7, 8, 9, 24, 25, 63, 64, 65, 96, 97, 128, 129, 255, 256, 257, 300):
        assert n in S.SUM_COUNTS
    assert S.SUM_COUNTS[0:2] == [257, 0] and S.SUM_COUNTS[15:17] == [0, 300]
    dead = S.only_past_256(c)
    fwd, ref = S.op_reference("counts-sum")
    assert dead.any()
    for name in S.OP_GRADS:
        assert not ref[name][dead].any()
    for t in (0, 16):  # the tiles past 256 keep pairs on both sides of every chunk
        keep = fwd["tiles"][t]["keep"]
        assert keep.shape[1] == 256 and all(keep[:, k:k + 64].any() for k in (0, 64, 128, 192))
    assert (c["opacity"] < 0.95).all()  # non-unit opacities
    for cid in S.OP_COUNT_IDS:
        assert (S.op_case(cid)["counts"] > S.TILE_PIX).any()


# ---------------------------------------------------------------- the restatements and the bars
def test_bars_are_four_times_worst():
    assert set(S.BARS) == set(S.WORST)
    for k, v in S.WORST.items():
        assert v > 0 and S.BARS[k] == 4.0 * v


@pytest.mark.parametrize("cid", S.OP_IDS)
def test_op_restatements_inside_worst(cid, oracle):
    """The C oracle and the sequential float32 restatement against float64:
    final_idx equal; the oracle inside 1.25 x WORST (recorded to three digits
    on one CPU; libm's exp2f has FMA and non-FMA variants), the numpy
    restatement inside twice WORST, half the bar (numpy's float32 exp is a SIMD
    routine that may differ in the last place from one CPU to another)."""
    c = S.op_case(cid)
    for run, room in ((S.oracle_op, 1.25), (S.float32_op, 2.0)):
        e = S.op_errors(cid, *run(c))
        assert e["idx"] == 0
        for k in ("image",) + S.OP_GRADS:
            assert S.worst_of(e, k) <= room * S.WORST[k], (run.__name__, k, e[k])


@pytest.mark.parametrize("cid", S.FUSED_IDS)
def test_fused_restatements_inside_worst(cid, oracle):
    p, r = S.fused_case(cid)
    for run, room in ((S.oracle_fused, 1.25), (S.float32_fused, 2.0)):
        e = S.fused_errors(cid, *run(p))
        for k in FUSED_KEYS:
            assert S.worst_of(e, k) <= room * S.WORST[k], (run.__name__, k, e[k])
