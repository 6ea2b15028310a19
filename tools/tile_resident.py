"""Resident workgroups per CU over the training tile kernel's life, from the
band kernel's per-tile stamps (Knob.STAMP = 3: st[0] start, st[4] end, st[6]
entries, st[7] = XCC_ID << 32 | HW_ID).

    python tools/tile_resident.py --capture OUT.npy [--warm 30]              # GPU
    python tools/tile_resident.py --analyze OUT.npy                          # anywhere

--capture trains the bench's frame (tests/golden/train_state_1080p_n50k.npz)
for --warm carried steps, stamps one step and saves the raw int64[ntiles][8].
--analyze prints one JSON line: workgroups resident per CU (maximum, by CU),
ramp, the dip between a CU's first and second generation, drain, slot fill.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def capture(path, warm):
    os.environ.setdefault("GSVC_DIAG", "1")
    import ctypes

    import torch
    from gsvc_amd import _lib
    from gsvc_amd.frame import make_frame_model, synthetic_gt
    from gsvc_amd.knobs import Knob
    z = np.load(os.path.join(REPO, "tests", "golden", "train_state_1080p_n50k.npz"))
    dev = torch.device("cuda:0")
    H, W = 1080, 1920
    m = make_frame_model(H, W, int(z["n"]), dev, seed=0)
    with torch.no_grad():
        for k in ("_xyz", "_cholesky", "_features_dc"):
            getattr(m, k).copy_(torch.from_numpy(z["state_" + k]))
    gt = synthetic_gt(H, W, int(z["gt_seed"]), dev)
    lib = _lib.load()
    for it in range(1, warm + 1):
        m.train_iter(gt, it)
    torch.cuda.synchronize()
    ntiles = ((W + 15) // 16) * ((H + 15) // 16)
    st = torch.zeros((ntiles, 8), dtype=torch.int64, device=dev)
    lib.gsvc_debug_set_ptr(ctypes.c_void_p(st.data_ptr()))
    lib.gsvc_debug_set(Knob.STAMP, 3)
    m.train_iter(gt, warm + 1)
    torch.cuda.synchronize()
    lib.gsvc_debug_set(Knob.STAMP, 0)
    lib.gsvc_debug_set_ptr(None)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.save(path, st.cpu().numpy())
    print(json.dumps(dict(saved=path, tiles=ntiles)), flush=True)


def analyze(raw, name="stamps"):
    """The figures of one stamped launch (``raw``: int64 [tiles, 8]) as a dict."""
    raw = np.asarray(raw)
    raw = raw[raw[:, 4] > 0]
    t0 = raw[:, 0].min()
    s = (raw[:, 0] - t0) * 0.01  # 100 MHz -> us
    e = (raw[:, 4] - t0) * 0.01
    hw = raw[:, 7]
    cu = ((hw >> 32) << 8) | ((hw >> 8) & 0xff)  # XCC, SE / SH / CU
    q = lambda x: [round(float(np.percentile(x, p)), 2) for p in (0, 10, 50, 90, 100)]  # noqa: E731
    end = float(e.max())
    cus = np.unique(cu)
    peak, ramp, dip_w, dip_lost, refill = [], [], [], [], []
    lost_total = 0.0
    for c in cus:
        sel = cu == c
        ev = sorted([(t, 1) for t in s[sel]] + [(t, -1) for t in e[sel]], key=lambda x: (x[0], x[1]))
        res, cur, ts = [], 0, []
        for t, d in ev:
            cur += d
            ts.append(t)
            res.append(cur)
        res, ts = np.array(res), np.array(ts)
        pk = int(res.max())
        peak.append(pk)
        at = np.nonzero(res == pk)[0]
        ramp.append(float(ts[at[0]]))
        # the dip: from the first end to the CU's return to its peak
        first_end = float(e[sel].min())
        back = at[ts[at] > first_end]
        if len(back):
            dip_w.append(float(ts[back[0]]) - first_end)
            k0, k1 = np.searchsorted(ts, first_end), back[0]
            dip_lost.append(float(np.sum((pk - res[k0:k1]) * np.diff(ts[k0:k1 + 1]))))
        lost_total += float(np.sum((pk - res[:-1]) * np.diff(ts))) + pk * (end - ts[-1]) + pk * ts[0]
        # a freed slot's wait for its next workgroup
        ss, ee = np.sort(s[sel]), np.sort(e[sel])
        later = ss[pk:]
        refill += list(later - ee[:len(later)])
    total_ev = sorted([(t, 1) for t in s] + [(t, -1) for t in e], key=lambda x: (x[0], x[1]))
    cur, tot_t, tot_r = 0, [], []
    for t, d in total_ev:
        cur += d
        tot_t.append(t)
        tot_r.append(cur)
    tot_t, tot_r = np.array(tot_t), np.array(tot_r)
    # the order phase (st[1] - st[0]) of every tile, and of each CU's first
    # generation -- its first `peak` workgroups by start -- by wave 0's slot
    order = (raw[:, 1] - raw[:, 0]) * 0.01
    gen1 = np.zeros(len(raw), dtype=bool)
    for c, pk in zip(cus, peak):
        idx = np.nonzero(cu == c)[0]
        gen1[idx[np.argsort(s[idx], kind="stable")[:pk]]] = True
    slot = hw & 15
    order_gen1_by_slot = {int(k): [round(float(np.percentile(order[gen1 & (slot == k)], p)), 2)
                                   for p in (10, 50, 90)] for k in np.unique(slot[gen1])}
    full = np.nonzero(tot_r >= 0.95 * tot_r.max())[0]
    cap = float(np.sum(peak)) * end
    # the drain starts when the chip last falls below 95 % of its peak
    fall = min(full[-1] + 1, len(tot_t) - 1)
    return dict(
        file=name, tiles=int(len(raw)), cus=int(len(cus)), kernel_us=round(end, 2),
        peak_resident_per_cu=dict(zip(*[x.tolist() for x in np.unique(peak, return_counts=True)])),
        peak_resident_total=int(tot_r.max()),
        ramp_to_peak_us=q(ramp), ramp_to_95pct_total_us=round(float(tot_t[full[0]]), 2),
        life_us=q(e - s), gen_dip_width_us=q(dip_w) if dip_w else None,
        gen_dip_lost_slot_us_per_cu=q(dip_lost) if dip_lost else None,
        slot_refill_wait_us=q(refill) if refill else None,
        drain_us=round(end - float(tot_t[fall]), 2),
        slot_fill=round(1.0 - lost_total / cap, 4),
        entries=q(raw[:, 6]),
        order_us=q(order), order_gen1_us=q(order[gen1]),
        order_gen1_us_p10_p50_p90_by_wave_slot=order_gen1_by_slot)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--capture", default=None)
    ap.add_argument("--analyze", default=None)
    ap.add_argument("--warm", type=int, default=30)
    a = ap.parse_args()
    if a.capture:
        capture(a.capture, a.warm)
    if a.analyze:
        print(json.dumps(analyze(np.load(a.analyze), os.path.basename(a.analyze))), flush=True)


if __name__ == "__main__":
    main()
