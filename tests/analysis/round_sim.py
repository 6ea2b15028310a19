"""What the backward rounds of the band kernel (train.hip, train_tile_band_kernel
step 4) work on at the bench's settled frame, rebuilt on the CPU from the
trained-state fixture alone (tests/golden/train_state_1080p_n50k.npz: the
parameters after 2000 iterations): every (splat, tile) rectangle, the items
each 8-row band makes of them, the rounds of 64 items, and the pixel-loop trips
of a round (its longest item) under the kernel's four length classes, under
an exact sort by length, and with every row trimmed to its alpha >= 1/255 span.

    python tests/analysis/round_sim.py [--tiles K]     # every K-th tile (default: all)

The figures DESIGN.md section 6 quotes: M (splat, tile) pairs, rectangle pixels,
items and entries per band, rounds per launch, wave-level loop trips per layout.
Reads nothing but the fixture; float64 restatements of project2d.h and rows.h.
"""
from __future__ import annotations

import argparse
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(os.path.dirname(HERE), "golden", "train_state_1080p_n50k.npz")
TILE = 16
S2 = 2.0 * (math.log(255.0) * 1.001 + 0.01)


def project(xyz, chol, H, W):
    """Centres, conics and tile boxes (x0, x1, y0, y1; exclusive ends) of the splats."""
    m = np.tanh(xyz.astype(np.float64))
    L = chol.astype(np.float64) + np.array([0.5, 0.0, 0.5])
    cx, cy = 0.5 * W * m[:, 0] + 0.5 * W, 0.5 * H * m[:, 1] + 0.5 * H
    cxx, cxy, cyy = L[:, 0] ** 2, L[:, 0] * L[:, 1], L[:, 1] ** 2 + L[:, 2] ** 2
    det = cxx * cyy - cxy ** 2
    ok = det != 0
    inv = np.where(ok, 1.0 / np.where(ok, det, 1.0), 0.0)
    conic = np.stack([cyy * inv, -cxy * inv, cxx * inv], 1)
    b = 0.5 * (cxx + cyy)
    r = np.ceil(3.0 * np.sqrt(b + np.sqrt(np.maximum(0.1, b * b - det))))
    tbx, tby = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    box = np.stack([np.clip(np.trunc((cx - r) / 16), 0, tbx), np.clip(np.trunc((cx + r) / 16 + 1), 0, tbx),
                    np.clip(np.trunc((cy - r) / 16), 0, tby), np.clip(np.trunc((cy + r) / 16 + 1), 0, tby)], 1)
    box[~ok] = 0
    return np.stack([cx, cy], 1), conic, box.astype(np.int64), tbx, tby


def rect(xy, conic, tx0, ty0):
    """rows.h ellipse_rect at opacity 1: inclusive x0, x1, y0, y1 and whether any."""
    a, b, c = conic[:, 0], conic[:, 1], conic[:, 2]
    det = a * c - b * b
    ex = np.sqrt(S2 * c / det) * 1.001 + 0.01
    ey = np.sqrt(S2 * a / det) * 1.001 + 0.01
    x0, x1 = np.maximum(np.ceil(xy[:, 0] - ex - tx0), 0), np.minimum(np.floor(xy[:, 0] + ex - tx0), 15)
    y0, y1 = np.maximum(np.ceil(xy[:, 1] - ey - ty0), 0), np.minimum(np.floor(xy[:, 1] + ey - ty0), 15)
    return x0.astype(int), x1.astype(int), y0.astype(int), y1.astype(int), (x0 <= x1) & (y0 <= y1)


def trips(lengths, order):
    """Loop trips of the rounds of 64 items laid out in `order`: each round's longest."""
    flat = lengths[order]
    return sum(int(flat[s:s + 64].max()) for s in range(0, flat.size, 64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=1, help="every K-th tile")
    a = ap.parse_args()
    z = np.load(FIXTURE)
    H, W = int(z["H"]), int(z["W"])
    xy, conic, box, tbx, tby = project(z["state__xyz"], z["state__cholesky"], H, W)
    area = (box[:, 1] - box[:, 0]) * (box[:, 3] - box[:, 2])
    print(f"M = {int(area.sum())} (splat, tile) pairs; the fixture records {int(z['M'])}")
    lists = [[] for _ in range(tbx * tby)]
    for i in np.flatnonzero(area > 0):
        for ty in range(box[i, 2], box[i, 3]):
            for tx in range(box[i, 0], box[i, 1]):
                lists[ty * tbx + tx].append(i)
    tot = dict(rect_px=0, pass_px=0, bands=0, items=0, entries=0, with_items=0, rounds=0, single=0,
               t_cls=0, t_sort=0, t_trim=0)
    for t in range(0, tbx * tby, a.tiles):
        ids = np.asarray(lists[t][:256], np.int64)
        if ids.size == 0:
            continue
        ty, tx = divmod(t, tbx)
        x0, x1, y0, y1, ok = rect(xy[ids], conic[ids], 16.0 * tx, 16.0 * ty)
        for band in (0, 1):
            tot["bands"] += 1
            for c0 in range(0, ids.size, 64):  # a chunk of 64 entries
                s = slice(c0, c0 + 64)
                r0, r1 = np.maximum(y0[s], 8 * band), np.minimum(y1[s], 8 * band + 7)
                has = ok[s] & (r0 <= r1)
                tot["entries"] += int(has.size)
                tot["with_items"] += int(has.sum())
                if not has.any():
                    continue
                wid = (x1[s] - x0[s] + 1)[has]
                rows = (r1 - r0 + 1)[has]
                e = np.repeat(np.arange(wid.size), rows)           # item -> entry
                length = wid[e]
                # the row's span with alpha >= 1/255 (sigma <= ln 255), per item
                k = np.flatnonzero(has)
                row = np.concatenate([np.arange(a0, a1 + 1) for a0, a1 in zip(r0[has], r1[has])])
                g = ids[s][k][e]
                dy = xy[g, 1] - (16.0 * ty + row)
                px = 16.0 * tx + np.arange(16)[None, :]
                dx = xy[g, 0][:, None] - px
                sg = 0.5 * (conic[g, 0][:, None] * dx * dx + conic[g, 2][:, None] * dy[:, None] ** 2) \
                    + conic[g, 1][:, None] * dx * dy[:, None]
                inside = (np.arange(16)[None, :] >= x0[s][k][e][:, None]) & (np.arange(16)[None, :] <= x1[s][k][e][:, None])
                hit = inside & (sg >= 0) & (np.exp(-sg) >= 1.0 / 255.0) & (16 * tx + np.arange(16)[None, :] < W)
                first = np.where(hit.any(1), hit.argmax(1), 0)
                last = np.where(hit.any(1), 15 - hit[:, ::-1].argmax(1), -1)
                trimmed = last - first + 1
                tot["rect_px"] += int(length.sum())
                tot["pass_px"] += int(hit.sum())
                n = int(rows.sum())
                tot["items"] += n
                tot["rounds"] += (n + 63) // 64
                tot["single"] += int(n <= 64)
                cls = np.where(wid >= 9, 3, np.where(wid >= 7, 2, np.where(wid >= 5, 1, 0)))
                by_cls = np.argsort(-cls[e], kind="stable")
                tot["t_cls"] += trips(length, by_cls)
                tot["t_sort"] += trips(length, np.argsort(-length, kind="stable"))
                tot["t_trim"] += trips(trimmed, by_cls)
    k = a.tiles
    print(f"rectangle pixels {tot['rect_px'] * k / 1e6:.2f} M, of which alpha >= 1/255: "
          f"{100.0 * tot['pass_px'] / tot['rect_px']:.1f} %")
    print(f"per band: {tot['items'] / tot['bands']:.1f} items, {tot['entries'] / tot['bands']:.1f} entries "
          f"({tot['with_items'] / tot['bands']:.1f} with items in the band)")
    print(f"rounds per launch {tot['rounds'] * k / 1e3:.1f} k ({tot['rounds'] / tot['bands']:.2f} per wave); "
          f"chunks of a single round: {100.0 * tot['single'] / tot['bands']:.1f} % of the bands")
    print(f"wave-level loop trips: four classes {tot['t_cls'] * k / 1e3:.0f} k; exact sort "
          f"{tot['t_sort'] * k / 1e3:.0f} k ({100.0 * (tot['t_sort'] / tot['t_cls'] - 1):+.1f} %); rows trimmed to the "
          f"alpha span {tot['t_trim'] * k / 1e3:.0f} k ({100.0 * (tot['t_trim'] / tot['t_cls'] - 1):+.1f} %)")


if __name__ == "__main__":
    main()
