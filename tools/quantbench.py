"""One quantized training iteration of the compression stage, op by op
(``train_iter_quantize``) against fused (``train_iter_quantize_fused``, one
``gsvc_quant_train_step`` call) against runs (``train_run_quantize_fused``, K
iterations per ``gsvc_quant_train_run`` call with the best state kept on the
device), in the same session: the 1920x1080 / 50k key frame of
tests/golden/train_state_1080p_n50k.npz with its quantizers initialised, and a
random-init delta frame on it (timing only).

    python tools/quantbench.py [--iters 100] [--windows 5] [--warmup 10]
                               [--methods op_by_op fused run] [--run 64 [K ...]]
    python tools/quantbench.py --end-to-end [--e2e-iters 2000] [--run 64] [--repeats 3]

Every method has its own model; after each one's warm-up the methods take
their windows in turn, window by window.  A ``run`` window is
max(1, round(iters / K)) calls of K iterations (one line per K, method
``run<K>``).

Per frame kind and method, one JSON line with
  wall_us        wall clock per iteration (the loop of compress_video: the
                 iteration ends in its loss read-back), --warmup iterations,
                 then --windows windows of --iters: [median, min, max]
  event_us       HIP events around the same windows, per iteration
and for the fused method
  call_event_us  HIP events around --iters gsvc_quant_train_step calls enqueued
                 back to back without the read-back: the C call's device time
and a last line with the ratio op-by-op / fused of the wall clock medians and
its [min, max] over the windows' pairs.  ``--end-to-end`` times
``compress_video`` itself on the key frame and one delta frame,
``fused=True`` against ``fused=True, run=K`` in turn, --repeats times: total
seconds on the host clock, ending in a synchronise, and from the single-step
loop the share of iterations at which its ``deepcopy`` of the best state fires.
A kernel trace is a run of its own:

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


def window(fn, calls, per_call, dev):
    """One window of ``calls`` calls of ``per_call`` iterations: (wall, event)
    microseconds per iteration."""
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = time.perf_counter()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    n = calls * per_call
    return 1e6 * (time.perf_counter() - t) / n, 1e3 * e0.elapsed_time(e1) / n


def windows(fn, a, dev):
    """(wall, event) microseconds per iteration, one value per window."""
    for _ in range(a.warmup):
        fn()
    pairs = [window(fn, a.iters, 1, dev) for _ in range(a.windows)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def end_to_end(a, dev):
    """compress_video on the key frame and one delta frame, single steps against runs."""
    import types
    z = np.load(os.path.join(REPO, "tests", "golden", "train_state_1080p_n50k.npz"))
    names = ("_xyz", "_cholesky", "_features_dc")
    key = {k: torch.from_numpy(z["state_" + k]).to(dev) for k in names}
    torch.manual_seed(1)
    nxt = {k: v + s * torch.randn_like(v) for (k, v), s in zip(key.items(), (0.01, 0.02, 0.02))}
    sd = {"frame_1": key, "frame_2": nxt}
    seed = int(z["gt_seed"])
    frames = [synthetic_gt(H, W, seed, "cpu").to(dev), synthetic_gt(H, W, seed + 1, "cpu").to(dev)]
    kw = dict(K_frames=[1], iterations=a.e2e_iters, lr=1e-3, device=dev, delta_base="decoded", seed=0,
              fused=True)
    fired = [0]
    real = C.copy

    def counting(x):
        fired[0] += 1
        return real.deepcopy(x)

    C.compress_video(sd, frames, **dict(kw, iterations=a.warmup), run=None)
    C.compress_video(sd, frames, **dict(kw, iterations=a.warmup), run=a.run[0])
    secs = {"fused": [], f"run{a.run[0]}": []}
    psnr = {}
    for _ in range(a.repeats):
        for name, run in (("fused", None), (f"run{a.run[0]}", a.run[0])):
            torch.cuda.synchronize(dev)
            t = time.perf_counter()
            out = C.compress_video(sd, frames, run=run, **kw)
            torch.cuda.synchronize(dev)
            secs[name].append(time.perf_counter() - t)
            psnr[name] = out["psnr"]
    for name, v in secs.items():
        print(json.dumps({"end_to_end": name, "frames": 2, "iterations_per_frame": a.e2e_iters,
                          "seconds": [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)],
                          "psnr": [round(p, 4) for p in psnr[name]]}), flush=True)
    # how often the single-step loop copies its best state (counted in a pass of its own)
    C.copy = types.SimpleNamespace(deepcopy=counting)
    try:
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        C.compress_video(sd, frames, run=None, **kw)
        torch.cuda.synchronize(dev)
        counted = time.perf_counter() - t
    finally:
        C.copy = real
    print(json.dumps({"end_to_end": "fused", "deepcopy_fired": fired[0],
                      "iterations": 2 * a.e2e_iters,
                      "share": round(fired[0] / (2 * a.e2e_iters), 4), "seconds": round(counted, 3)}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--methods", nargs="+", default=["op_by_op", "fused"],
                    choices=["op_by_op", "fused", "run"])
    ap.add_argument("--run", nargs="+", type=int, default=[64], metavar="K",
                    help="iterations per call of the run method (several: one line each)")
    ap.add_argument("--end-to-end", action="store_true", help="time compress_video instead")
    ap.add_argument("--e2e-iters", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("quantbench: no HIP device; nothing is measured without one")
    dev = torch.device("cuda:0")
    if a.end_to_end:
        end_to_end(a, dev)
        return
    for delta in (False, True):
        # per method: its model's call, the calls per window, the iterations per call
        plan = []
        for method in a.methods:
            for k in (a.run if method == "run" else [1]):
                m, gt_seed = model(dev, delta)
                gt = synthetic_gt(H, W, gt_seed, "cpu").to(dev)
                psnr = []
                if method == "run":
                    best = C.QuantBestState(m)
                    fn = (lambda m=m, gt=gt, k=k, best=best, psnr=psnr:
                          psnr.extend(m.train_run_quantize_fused(gt, k, best)[1]))
                    calls = max(1, round(a.iters / k))
                    for _ in range(max(1, -(-a.warmup // k))):
                        fn()
                else:
                    it = m.train_iter_quantize_fused if method == "fused" else m.train_iter_quantize
                    fn = lambda it=it, gt=gt, psnr=psnr: psnr.append(it(gt)[1])  # noqa: E731
                    calls = a.iters
                    for _ in range(a.warmup):
                        fn()
                plan.append(dict(name=method + (str(k) if method == "run" else ""), m=m, gt=gt, fn=fn,
                                 calls=calls, k=k, psnr=psnr, wall=[], ev=[]))
        for _ in range(a.windows):  # the methods in turn, window by window
            for p in plan:
                w, e = window(p["fn"], p["calls"], p["k"], dev)
                p["wall"].append(w)
                p["ev"].append(e)
        walls = {}
        for p in plan:
            m, psnr = p["m"], p["psnr"]
            walls[p["name"]] = p["wall"]
            line = {"frame": "delta" if delta else "key", "method": p["name"], "splats": m._xyz.shape[0],
                    "wall_us": stats(p["wall"]), "event_us": stats(p["ev"]),
                    "psnr_first_last": [round(psnr[0], 3), round(psnr[-1], 3)]}
            if p["name"] == "fused":
                bs = m._bound_quant_step
                hp = list(bs.hp)
                gtc = p["gt"].contiguous()
                _, call = windows(lambda: bs.step(gtc, hp, 0, sync=False), a, dev)
                line["call_event_us"] = stats(call)
            if p["name"].startswith("run"):
                line["iterations_per_window"] = p["calls"] * p["k"]
            print(json.dumps(line), flush=True)
        if "fused" in walls:
            for name, wall in walls.items():
                if name.startswith("run"):
                    print(json.dumps({"frame": "delta" if delta else "key", "method": name,
                                      "median_wall_us": round(statistics.median(wall), 1),
                                      "fused_min_window_us": round(min(walls["fused"]), 1),
                                      "below_fused_min": statistics.median(wall) < min(walls["fused"])}),
                          flush=True)
        if "op_by_op" not in walls or "fused" not in walls:
            continue
        ratios = [o / f for o, f in zip(walls["op_by_op"], walls["fused"])]
        print(json.dumps({"frame": "delta" if delta else "key",
                          "op_by_op_over_fused_wall": round(statistics.median(walls["op_by_op"])
                                                            / statistics.median(walls["fused"]), 2),
                          "window_ratios_min_max": [round(min(ratios), 2), round(max(ratios), 2)]}),
              flush=True)


if __name__ == "__main__":
    main()
