"""Where the bars of tests/sum_cases.py come from: two float32 restatements
against the float64 references of tests/sum_cases.py over every case -- the C
oracle (forward.cu:512-627 / backward.cu:696-862 / foward2d.cu / backward2d.cu
in float32, sums in double) and sum_cases.chain_np in float32 with every sum
taken sequentially in float32 in pixel order (the least favourable honest
summation: it covers the kernels' DPP trees and float atomics).  Worst error
per quantity: image and losses absolute (losses also relative), each gradient
relative to the reference's largest element -- the worst of the whole tensor,
the edge subset and, on the counts cases, each tile's own splats.  The
kernels' bar is 4 times the worse of the two figures.  The tile grids of
tests/grid_cases.py are measured last and reported apart (sum_cases.WORST_GRID):
their float32 losses use publish_loss's summation (float32 inside a tile,
float64 across tiles), and what exceeds WORST there is the wide frames' input
rounding, which must not loosen the bars of the small cases.

    python tests/analysis/sum_bars.py
"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle")):
    sys.path.insert(0, p)

import grid_cases as G  # noqa: E402
import sum_cases as S  # noqa: E402

OP_KEYS = ("image",) + S.OP_GRADS
FUSED_KEYS = ("render", "loss_abs", "loss_rel") + tuple(n for n, _ in S.PARAM_GRADS)


def measure():
    """{restatement: {quantity: (worst, case)}} over every case."""
    worst = {w: {} for w in ("oracle", "float32-seq")}
    grid = {w: {} for w in ("oracle", "float32-seq")}  # tests/grid_cases.py, kept apart (WORST_GRID)

    def note(who, key, val, cid, into=None):
        into = worst if into is None else into
        if val > into[who].get(key, (-1.0, ""))[0]:
            into[who][key] = (val, cid)

    for cid in S.OP_IDS:
        c = S.op_case(cid)
        line = f"{cid:14s} op    nudged {c['nudged']:2d}"
        for who, run in (("oracle", S.oracle_op), ("float32-seq", S.float32_op)):
            e = S.op_errors(cid, *run(c))
            assert e["idx"] == 0, (cid, who)
            for k in OP_KEYS:
                note(who, k, S.worst_of(e, k), cid)
            line += f" | {who} " + " ".join(f"{S.worst_of(e, k):8.2e}" for k in OP_KEYS)
        print(line)
    for cid in S.FUSED_IDS:
        p, r = S.fused_case(cid)
        line = f"{cid:14s} fused nudged {p['nudged']:2d}"
        for who, run in (("oracle", S.oracle_fused), ("float32-seq", S.float32_fused)):
            e = S.fused_errors(cid, *run(p))
            for k in FUSED_KEYS:
                note(who, k, S.worst_of(e, k), cid)
            line += f" | {who} " + " ".join(f"{S.worst_of(e, k):8.2e}" for k in FUSED_KEYS)
        print(line)
    # the tile grids of tests/grid_cases.py: the op-level view of each rendered
    # grid (image only: the fused step carries the gradients) and the fused
    # step, the float32 restatement with publish_loss's summation (float32
    # inside a tile, float64 across tiles) and the per-tile gradient measure
    for cid in G.FORWARD_IDS:
        c = G.op_case(cid)
        keep = ~c["fwd"]["borderline"]
        line = f"{cid:14s} op    masked {int((~keep).sum()):2d}"
        for who, run in (("oracle", S.oracle_op_forward), ("float32-seq", S.float32_op_forward)):
            out, idx = run(c)
            assert (idx[keep] == c["fwd"]["idx"][keep]).all(), (cid, who)
            e = S.image_error(out, c["fwd"]["out"], keep)
            note(who, "image", e, cid, grid)
            line += f" | {who} {e:8.2e}"
        print(line)
    for cid in G.GRID_IDS:
        p, r = G.grid_case(cid)
        line = f"{cid:14s} fused nudged {p['nudged']:2d}"
        for who, run in (("oracle", S.oracle_fused), ("float32-seq", G.float32_fused)):
            e = G.grid_errors(cid, *run(p))
            for k in FUSED_KEYS:  # the fused step runs on STEP_IDS; the clamped render on every grid
                if cid in G.STEP_IDS or k == "render":
                    note(who, k, S.worst_of(e, k), cid, grid)
            line += f" | {who} " + " ".join(f"{S.worst_of(e, k):8.2e}" for k in FUSED_KEYS)
        print(line)
    return worst, grid


def main():
    t0 = time.time()
    worst, grid = measure()
    print(f"\n{time.time() - t0:.1f} s")
    keys = list(dict.fromkeys(OP_KEYS + FUSED_KEYS))
    print(f"{'':12s} {'oracle':>10s} {'case':14s} {'float32-seq':>11s} {'case':14s} {'bar':>10s}")
    for k in keys:
        (a, ca), (b, cb) = worst["oracle"][k], worst["float32-seq"][k]
        print(f"{k:12s} {a:10.2e} {ca:14s} {b:11.2e} {cb:14s} {4 * max(a, b):10.2e}")
    print("WORST = dict(" + ", ".join(
        f"{k}={max(worst['oracle'][k][0], worst['float32-seq'][k][0]):.2e}" for k in keys) + ")")
    print("\nthe tile grids (WORST_GRID lists what exceeds WORST)")
    over = {}
    for k in keys:
        if k in grid["oracle"]:
            (a, ca), (b, cb) = grid["oracle"][k], grid["float32-seq"][k]
            top = max(worst["oracle"][k][0], worst["float32-seq"][k][0])
            print(f"{k:12s} {a:10.2e} {ca:14s} {b:11.2e} {cb:14s} {4 * max(a, b, top):10.2e}")
            if max(a, b) > top:
                over[k] = max(a, b)
    print("WORST_GRID = dict(" + ", ".join(f"{k}={v:.2e}" for k, v in over.items()) + ")")


if __name__ == "__main__":
    main()
