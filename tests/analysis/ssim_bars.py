"""Where the bars of tests/test_ssim_edges.py come from: the fp32 torch
restatement of SSIM / MS-SSIM on the CPU against the float64 reference, over
every case of tests/ssim_cases.py, worst error per tolerance family (value:
absolute; gradient: relative to the reference's largest element, whole tensor
and outer band).  The kernels' bar is 4 times the worst figure of the family.

    python tests/analysis/ssim_bars.py

Also checks the references against each other: `reference` (per-plane terms,
clamped planes left out) equals t_ssim / t_ms_ssim in float64 wherever nothing
clamps, and its value equals the numpy oracle's.
"""
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import oracle as O  # noqa: E402
import ssim_cases as S  # noqa: E402


def main():
    warnings.simplefilter("ignore")
    worst = {}
    print(f"{'case':14s} {'family':6s} {'value':>9s} {'dX whole':>9s} {'dX band':>9s} "
          f"{'dY whole':>9s} {'dY band':>9s}")
    for c in S.CASES:
        win = c["opts"].get("win_size", 11)
        r64 = S.reference(c)
        r32 = S.reference(c, dtype=torch.float32)
        # the references agree with each other
        ov = S.oracle_value(O, c)
        assert np.abs(r64["value"].numpy() - ov).max() < 1e-11 * max(1.0, np.abs(ov).max()), c["id"]
        if not r64["clamped"].any():
            lv, lx, ly = S.library_reference(c)
            assert float((lv - r64["value"]).abs().max()) < 1e-12, c["id"]
            assert float((lx - r64["dX"]).abs().max()) <= 1e-12 * float(lx.abs().max()), c["id"]
            assert float((ly - r64["dY"]).abs().max()) <= 1e-12 * float(ly.abs().max()), c["id"]
        assert torch.equal(r32["clamped"], r64["clamped"]), c["id"]
        keep = ~r64["clamped"]
        ev = float((r32["value"].double() - r64["value"]).abs().max())
        ex = S.grad_errors(r32["dX"], r64["dX"], win, keep)
        ey = S.grad_errors(r32["dY"], r64["dY"], win, keep)
        print(f"{c['id']:14s} {c['family']:6s} {ev:9.2e} {ex[0]:9.2e} {ex[1]:9.2e} {ey[0]:9.2e} "
              f"{ey[1]:9.2e}")
        w = worst.setdefault(c["family"], [0.0, 0.0, 0.0])
        w[0] = max(w[0], ev)
        w[1] = max(w[1], ex[0], ey[0])
        w[2] = max(w[2], ex[1], ey[1])
    # X is Y: the fp32 restatement's gradient against 0, relative to the noisy
    # pair's largest reference element at the same shape
    c = S.BY_ID["t-27x75"]
    scale = float(S.reference(c)["dX"].abs().max())
    X = S.inputs(c)[0].requires_grad_(True)
    out = S.t_ssim(X, X, size_average=False)
    (out * S.upstream(out.numel(), torch.float32)).sum().backward()
    print(f"X is Y: value {out.tolist()}, |grad| / scale = {float(X.grad.abs().max()) / scale:.2e}")
    print()
    for fam, (v, g, b) in worst.items():
        print(f"{fam:6s} value {v:.2e}  gradient whole {g:.2e}  band {b:.2e}")


if __name__ == "__main__":
    main()
