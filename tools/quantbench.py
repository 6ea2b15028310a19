"""One quantized training iteration of the compression stage, op by op
(``train_iter_quantize``) against fused (``train_iter_quantize_fused``, one
``gsvc_quant_train_step`` call), in the same session: the 1920x1080 / 50k key
frame of tests/golden/train_state_1080p_n50k.npz with its quantizers
initialised, and a random-init delta frame on it (timing only).

    python tools/quantbench.py [--iters 100] [--windows 5] [--warmup 10] [--methods op_by_op fused]

Per frame kind and method, one JSON line with
  wall_us        wall clock per iteration (the loop of compress_video: the
                 iteration ends in its loss read-back), --warmup iterations,
                 then --windows windows of --iters: [median, min, max]
  event_us       HIP events around the same windows, per iteration
and for the fused method
  call_event_us  HIP events around --iters gsvc_quant_train_step calls enqueued
                 back to back without the read-back: the C call's device time
and a last line with the ratio op-by-op / fused of the wall clock medians and
its [min, max] over the windows' pairs.  A kernel trace is a run of its own:

    rocprofv3 --kernel-trace --stats -- python tools/quantbench.py --iters 20 --windows 1 --methods fused
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gsvc_amd import compress as C  # noqa: E402
from gsvc_amd.frame import synthetic_gt  # noqa: E402

H, W = 1080, 1920


def model(dev, delta):
    z = np.load(os.path.join(REPO, "tests", "golden", "train_state_1080p_n50k.npz"))
    n = int(z["n"])
    state = [torch.from_numpy(z[k]).to(dev) for k in ("state__xyz", "state__cholesky", "state__features_dc")]
    torch.manual_seed(0)
    m = (C.GaussianVideoDelta if delta else C.GaussianVideoFrameQ)(
        num_points=n, H=H, W=W, BLOCK_H=16, BLOCK_W=16, device=dev, lr=1e-3, quantize=True,
        opt_type="adan").to(dev)
    with torch.no_grad():
        if delta:
            m._xyz.copy_(0.05 * torch.randn(n, 2))
            m._cholesky.copy_(0.3 * torch.randn(n, 3))
            m._features_dc.copy_(0.1 * torch.randn(n, 3))
            for p, v in zip((m.p_xyz, m.p_cholesky, m.p_features_dc), state):
                p.copy_(v)
        else:
            for p, v in zip((m._xyz, m._cholesky, m._features_dc), state):
                p.copy_(v)
    m._init_data()
    return m.train(), int(z["gt_seed"])


def stats(v):
    return [round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)]


def windows(fn, a, dev):
    """(wall, event) microseconds per iteration, one value per window."""
    for _ in range(a.warmup):
        fn()
    wall, ev = [], []
    for _ in range(a.windows):
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = time.perf_counter()
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        wall.append(1e6 * (time.perf_counter() - t) / a.iters)
        ev.append(1e3 * e0.elapsed_time(e1) / a.iters)
    return wall, ev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--methods", nargs="+", default=["op_by_op", "fused"], choices=["op_by_op", "fused"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("quantbench: no HIP device; nothing is measured without one")
    dev = torch.device("cuda:0")
    for delta in (False, True):
        walls = {}
        for method in a.methods:
            m, gt_seed = model(dev, delta)
            gt = synthetic_gt(H, W, gt_seed, "cpu").to(dev)
            it = m.train_iter_quantize_fused if method == "fused" else m.train_iter_quantize
            psnr = []
            wall, ev = windows(lambda: psnr.append(it(gt)[1]), a, dev)
            walls[method] = wall
            line = {"frame": "delta" if delta else "key", "method": method, "splats": m._xyz.shape[0],
                    "wall_us": stats(wall), "event_us": stats(ev),
                    "psnr_first_last": [round(psnr[0], 3), round(psnr[-1], 3)]}
            if method == "fused":
                bs = m._bound_quant_step
                hp = list(bs.hp)
                gtc = gt.contiguous()
                _, call = windows(lambda: bs.step(gtc, hp, 0, sync=False), a, dev)
                line["call_event_us"] = stats(call)
            print(json.dumps(line), flush=True)
        if len(walls) < 2:
            continue
        ratios = [o / f for o, f in zip(walls["op_by_op"], walls["fused"])]
        print(json.dumps({"frame": "delta" if delta else "key",
                          "op_by_op_over_fused_wall": round(statistics.median(walls["op_by_op"])
                                                            / statistics.median(walls["fused"]), 2),
                          "window_ratios_min_max": [round(min(ratios), 2), round(max(ratios), 2)]}),
              flush=True)


if __name__ == "__main__":
    main()
