"""Where the bars of tests/alpha_cases.py come from: the C oracle (the float32
restatement of forward.cu:252-374 / backward.cu:138-315) against the float64
references of tests/alpha_cases.py over every float64 case, outside the
borderline mask: worst error per quantity (image, T: absolute; each gradient:
relative to the reference's largest element, the worse of the whole tensor and
the edge subset).  The kernels' bar is 4 times the worst figure.

    python tests/analysis/alpha_bars.py

Also prints per case the borderline share, the 0.99 mask's size and the
agreement of the two gradient references where that mask is empty.
"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

import alpha_cases as A  # noqa: E402


def main():
    worst = {k: 0.0 for k in A.WORST}
    t0 = time.time()
    print(f"{'case':16s} {'bord%':>6s} {'hi99':>5s} {'image':>9s} {'T':>9s} "
          + " ".join(f"{g:>19s}" for g in A.GRADS) + "  autograd-vs-recursion")
    for cid in A.F64_IDS:
        c = A.BY_ID[cid]
        r = A.reference(cid)
        fwd = r["fwd"]
        keep = ~fwd["borderline"]
        out, Ts, idx, g = A.oracle_run(c, r["v_out"], r["v_alpha"])
        assert np.array_equal(idx[keep], fwd["idx"][keep]), cid
        e_img = float(np.abs(out - fwd["out"])[keep].max())
        e_T = float(np.abs(Ts - fwd["T"])[keep].max())
        ge = A.grad_errors(c, g, r["rec"])
        worst["image"] = max(worst["image"], e_img)
        worst["T"] = max(worst["T"], e_T)
        for k, (w, e) in ge.items():
            worst[k] = max(worst[k], w, e)
        agree = ""
        if not fwd["hi99"].any():
            ag = A.alpha_backward64_autograd(c, fwd, r["v_out"], r["v_alpha"])
            agree = f"{max(A.rel_error(ag[k], r['rec'][k]) for k in A.GRADS):.1e}"
        print(f"{cid:16s} {100 * fwd['borderline'].mean():6.2f} {int(fwd['hi99'].sum()):5d} "
              f"{e_img:9.2e} {e_T:9.2e} "
              + " ".join(f"{ge[k][0]:9.2e} {ge[k][1]:9.2e}" for k in A.GRADS) + f"  {agree}")
    for cid, kind in A.VARIANT_IDS:
        c, fwd = A.BY_ID[cid], A.reference(cid)["fwd"]
        vo, va, fi, ref = A.variant(cid, kind)
        g = A.oracle_run(c, vo, va, fi)[3]
        ge = A.grad_errors(c, g, ref)
        for k, (w, e) in ge.items():
            worst[k] = max(worst[k], w, e)
        print(f"{cid + ' ' + kind:30s} {'':21s} "
              + " ".join(f"{ge[k][0]:9.2e} {ge[k][1]:9.2e}" for k in A.GRADS))
    print(f"\n{time.time() - t0:.1f} s")
    for k, v in worst.items():
        print(f"{k:10s} worst {v:.2e}  bar {4 * v:.2e}")


if __name__ == "__main__":
    main()
