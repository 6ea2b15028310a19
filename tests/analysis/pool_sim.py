"""The backward rounds of the band kernel (train.hip, train_tile_band_kernel
step 4) with the items of both bands of a tile pooled into one table, rebuilt
on the CPU from the trained-state fixture alone (round_sim.py's ``project`` /
``rect`` / ``trips``): wave-level pixel-loop trips and rounds per launch for

* the items per band (one table a wave) or per tile (one table, its rounds
  dealt to the two waves),
* four length classes (9+, 7-8, 5-6, <= 4), eight (widths 1-2, 3-4, ...,
  15-16) or an exact sort by length, stable in entry order,
* the pooled rounds dealt to the waves alternately (round r to wave r & 1) or
  as a snake (0, 1, 1, 0, ...): the trips of either wave, and of the longer
  one per tile (what the workgroup waits for),
* row pairs as one item (a later change: the figure only).

    python tests/analysis/pool_sim.py [--tiles K]     # every K-th tile (default: all)

Reads nothing but the fixture.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from round_sim import FIXTURE, project, rect, trips  # noqa: E402


def round_trips(lengths, order):
    """The trips of each round of 64 items laid out in `order`."""
    flat = lengths[order]
    return [int(flat[s:s + 64].max()) for s in range(0, flat.size, 64)]


def cls4(w):
    return np.where(w >= 9, 3, np.where(w >= 7, 2, np.where(w >= 5, 1, 0)))


def cls8(w):
    return (w - 1) >> 1


def snake_wave(r):
    return ((r + 1) >> 1) & 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=1, help="every K-th tile")
    a = ap.parse_args()
    z = np.load(FIXTURE)
    H, W = int(z["H"]), int(z["W"])
    xy, conic, box, tbx, tby = project(z["state__xyz"], z["state__cholesky"], H, W)
    area = (box[:, 1] - box[:, 0]) * (box[:, 3] - box[:, 2])
    lists = [[] for _ in range(tbx * tby)]
    for i in np.flatnonzero(area > 0):
        for ty in range(box[i, 2], box[i, 3]):
            for tx in range(box[i, 0], box[i, 1]):
                lists[ty * tbx + tx].append(i)
    names = ("band4", "band8", "bandx", "pool4", "pool8", "poolx", "pairs_band", "pairs_pool")
    t = {k: 0 for k in names}
    r = {k: 0 for k in names}
    items = pixels = tiles = 0
    hist = np.zeros(17, np.int64)
    deal = {"alternate": np.zeros(2, np.int64), "snake": np.zeros(2, np.int64)}
    deal_max = {"alternate": 0, "snake": 0}
    for tl in range(0, tbx * tby, a.tiles):
        ids = np.asarray(lists[tl][:256], np.int64)
        if ids.size == 0:
            continue
        tiles += 1
        ty, tx = divmod(tl, tbx)
        x0, x1, y0, y1, ok = rect(xy[ids], conic[ids], 16.0 * tx, 16.0 * ty)
        wave = {"alternate": np.zeros(2, np.int64), "snake": np.zeros(2, np.int64)}
        for c0 in range(0, ids.size, 64):  # a chunk of 64 entries
            s = slice(c0, c0 + 64)
            wid_all = x1[s] - x0[s] + 1
            for lo, hi, tag in ((0, 7, "band"), (8, 15, "band"), (0, 15, "pool")):
                r0, r1 = np.maximum(y0[s], lo), np.minimum(y1[s], hi)
                has = ok[s] & (r0 <= r1)
                if not has.any():
                    continue
                wid = wid_all[has]
                rows = (r1 - r0 + 1)[has]
                e = np.repeat(np.arange(wid.size), rows)  # item -> entry
                length = wid[e]
                for key, order in ((tag + "4", np.argsort(-cls4(wid)[e], kind="stable")),
                                   (tag + "8", np.argsort(-cls8(wid)[e], kind="stable")),
                                   (tag + "x", np.argsort(-length, kind="stable"))):
                    t[key] += trips(length, order)
                    r[key] += (length.size + 63) // 64
                # row pairs: one item = two rows of an entry, a trip covers both
                ep = np.repeat(np.arange(wid.size), (rows + 1) >> 1)
                t["pairs_" + tag] += trips(wid[ep], np.argsort(-cls8(wid)[ep], kind="stable"))
                r["pairs_" + tag] += (ep.size + 63) // 64
                if tag == "pool":
                    items += length.size
                    pixels += int(length.sum())
                    hist += np.bincount(length, minlength=17)
                    rt = round_trips(length, np.argsort(-cls8(wid)[e], kind="stable"))
                    for q, v in enumerate(rt):
                        wave["alternate"][q & 1] += v
                        wave["snake"][snake_wave(q)] += v
        for k in deal:
            deal[k] += wave[k]
            deal_max[k] += int(wave[k].max())
    k = a.tiles
    print(f"{tiles * k} tiles with entries, {items * k / 1e6:.2f} M items, {pixels * k / 1e6:.2f} M rectangle pixels")
    print("items by length 1..16 (k): " + " ".join(f"{v * k / 1e3:.0f}" for v in hist[1:]))
    print("layout                         trips / launch   rounds / launch")
    for key, name in (("band4", "per band, four classes"), ("band8", "per band, eight classes"),
                      ("bandx", "per band, exact sort"), ("pool4", "pooled, four classes"),
                      ("pool8", "pooled, eight classes"), ("poolx", "pooled, exact sort"),
                      ("pairs_band", "row pairs per band, eight"), ("pairs_pool", "row pairs pooled, eight")):
        print(f"{name:30s} {t[key] * k / 1e3:10.1f} k {r[key] * k / 1e3:14.2f} k"
              f"   ({100.0 * (t[key] / t['band4'] - 1):+.1f} %)")
    print(f"perfect packing (pixels / 64): {pixels * k / 64e3:.1f} k trips")
    for name in ("alternate", "snake"):
        d = deal[name] * k / 1e3
        print(f"pooled eight classes, {name:9s} deal: wave 0 {d[0]:.1f} k, wave 1 {d[1]:.1f} k trips; "
              f"the longer wave of each tile {deal_max[name] * k / 1e3:.1f} k")


if __name__ == "__main__":
    main()
