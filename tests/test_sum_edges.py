"""The sum rasteriser (gsvc_amd/csrc/raster_sum.hip) and the fused training
step (train.hip's tile and splat kernels) on the scripted cases of
tests/sum_cases.py: the per-tile entry counts, id ranges and rectangle shapes at
which the kernels change code path, partial tiles on both edges, and gradients
against float64 references that are not the kernels' own restatement.  Bars:
sum_cases.BARS (4 x the worse of two float32 restatements' worst errors against
float64, tests/analysis/sum_bars.py).  Every gradient is measured three ways:
over the whole tensor, over the splats near the right / bottom edge, and -- on
the counts cases -- per tile against the largest element among that tile's own
splats, the measure that can see a dense tile.  Every figure is printed before
it is asserted (``SUM-ERR`` lines; pytest -s shows them)."""
import contextlib
import math

import numpy as np
import pytest
import torch

import sum_cases as S
from conftest import knobs
from gsvc_amd.knobs import Knob

pytestmark = pytest.mark.gpu


def T(a, dev="cuda"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


@pytest.fixture(params=["band", "wg256"])
def tile_kernel(request, cuda):
    """The fused step's tile kernel: two 8-row band waves per tile (production)
    or the 256-thread workgroup per tile (Knob.TILE_WG256 = 1, the diagnostic
    library)."""
    with knobs((Knob.TILE_WG256, 1 if request.param == "wg256" else 0)):
        yield request.param


@contextlib.contextmanager
def deterministic():
    prev = torch.are_deterministic_algorithms_enabled()
    warn = torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev, warn_only=warn)


def _report(cid, what, name, value, bar):
    print(f"SUM-ERR {cid} {what} {name} {value:.3e} bar {bar:.3e}")


def _check(cid, what, errs, keys):
    """Print every figure of `errs`, then hold each to its bar."""
    flat = []
    for k in keys:
        v = errs[k]
        if isinstance(v, tuple):
            whole, edge, tile, where = v
            flat += [(k + ".whole", whole, k), (k + ".edge", edge, k), (f"{k}.tile[{where}]", tile, k)]
        else:
            flat.append((k, v, k))
    for name, val, k in flat:
        _report(cid, what, name, val, S.BARS[k])
    for name, val, k in flat:
        assert val <= S.BARS[k], (cid, what, name, val, S.BARS[k])


# ---------------------------------------------------------------- op level
def _tb(c):
    return ((c["W"] + 15) // 16, (c["H"] + 15) // 16, 1)


def _dev(c):
    d = [T(c[k]) for k in ("gids", "bins", "xys", "conics", "colors", "opacity")]
    return d + [torch.ones(3, device="cuda")]


def _forward(c, d):
    from gsvc_amd import ops
    return ops.rasterize_sum_forward(_tb(c), (16, 16, 1), (c["W"], c["H"], 1), *d)


@pytest.mark.parametrize("cid", S.OP_IDS)
def test_sum_op_against_float64(cuda, cid):
    """rasterize_sum_forward / _ex (every composite layout) / _backward on the
    kernel's own final_idx with v_out ~ N(0, 1): image, final_idx (exact off the
    borderline mask) and the four gradients against sum_forward64 /
    sum_backward64.  Past 256 entries the rest of a list adds exactly nothing
    to the image, and a splat listed only there gets an exactly zero row."""
    from gsvc_amd import ops
    c = S.op_case(cid)
    fwd, ref = S.op_reference(cid)
    keep = ~fwd["borderline"]
    d = _dev(c)
    out, Ts, idx = _forward(c, d)
    assert (N(Ts) == 1).all()
    args = (_tb(c), (16, 16, 1), (c["W"], c["H"], 1), *d)
    hwc, idx_ex = ops.rasterize_sum_forward_ex(*args, layout=ops.LAYOUT_HWC)
    planes, _ = ops.rasterize_sum_forward_ex(*args, layout=ops.LAYOUT_CHW, want_idx=False)
    clamped, _ = ops.rasterize_sum_forward_ex(*args, layout=ops.LAYOUT_CHW_CLAMPED, want_idx=False)
    e_layout = dict(hwc=S.image_error(N(hwc), fwd["out"], keep),
                    planes=S.image_error(N(planes).transpose(1, 2, 0), fwd["out"], keep),
                    clamped=S.image_error(N(clamped).transpose(1, 2, 0), np.clip(fwd["out"], 0, 1), keep))
    g = ops.rasterize_sum_backward(c["H"], c["W"], 16, 16, *d, None, idx, T(c["v_out"]), None)
    errs = S.op_errors(cid, N(out), N(idx), [N(t) for t in g])
    for name, val in e_layout.items():
        _report(cid, "op", "image." + name, val, S.BARS["image"])
    _check(cid, "op", errs, ("image",) + S.OP_GRADS)
    assert errs["idx"] == 0
    np.testing.assert_array_equal(N(idx_ex)[keep], fwd["idx"][keep])
    assert max(e_layout.values()) <= S.BARS["image"]
    assert torch.equal(planes, hwc.permute(2, 0, 1))
    if (c["counts"] > S.TILE_PIX).any():
        short = S.truncated(c)  # (its final_idx counts in the shorter id array: not compared)
        o2, _, _ = _forward(short, _dev(short))
        assert torch.equal(o2, out)
        dead = S.only_past_256(c)
        assert dead.any()
        for t in g:
            assert not N(t)[dead].any()


# ---------------------------------------------------------------- the fused step
def _step(p, dev):
    """train_step_sum with the test hooks: (render [3, H, W], losses [2],
    grads [N, 9]) as device tensors."""
    from gsvc_amd.train import train_step_sum
    n, H, W = p["xyz"].shape[0], p["H"], p["W"]
    g = torch.empty((n, 9), device=dev)
    render = torch.empty((1, 3, H, W), device=dev)
    losses = train_step_sum(T(p["xyz"]), T(p["chol"]), T(p["feat"]), T(p["rgbw"]), p["rgbw_train"],
                            T(p["bound"]).view(1, 3), T(p["bg"]), T(p["gt"]).view(1, 3, H, W), H, W,
                            p["loss"], render_out=render, grads_out=g)
    return render[0], losses, g


def _model(p, dev, **kw):
    """A GaussianVideoFrame holding the case's parameters."""
    from gsvc_amd.frame import make_frame_model
    m = make_frame_model(p["H"], p["W"], p["xyz"].shape[0], dev, seed=0, isremoval=p["rgbw_train"], **kw)
    m.loss_type = p["loss"]
    with torch.no_grad():
        m._xyz.copy_(T(p["xyz"]))
        m._cholesky.copy_(T(p["chol"]))
        m._features_dc.copy_(T(p["feat"]))
        m.rgb_W.copy_(T(p["rgbw"]))
        m.background.copy_(T(p["bg"]))
    return m


def _oracle_image(cid, p):
    # float64 does not decide 1 - tanh^2 at |xyz| >= 9: the image goes against
    # the float32 restatement, whose own distance from float64 is added
    return S.oracle_fused(p)[0].astype(np.float64) if cid == "saturated" else None


def _check_fused(cid, what, render, losses, g):
    p, r = S.fused_case(cid)
    ref_img = _oracle_image(cid, p)
    errs = S.fused_errors(cid, N(render), N(losses) if torch.is_tensor(losses) else losses, N(g), ref_img)
    if ref_img is not None:  # the triangle inequality: kernel-oracle <= kernel-float64 + oracle-float64
        _report(cid, what, "render(oracle)", errs["render"], S.BARS["render"] + S.WORST["render"])
        assert errs["render"] <= S.BARS["render"] + S.WORST["render"]
        errs["render"] = 0.0
    _check(cid, what, errs, ("render", "loss_abs", "loss_rel") + tuple(n for n, _ in S.PARAM_GRADS))
    if r["M"] < 1:
        assert not N(g).any()
    dead = ~r["proj"]["ok"]
    assert not N(g)[dead].any()  # a skipped (det = 0) splat: exactly zero


@pytest.mark.parametrize("cid", S.FUSED_IDS)
def test_fused_step_against_float64(cuda, tile_kernel, cid):
    """gsvc_train_step_sum (both tile kernels): the clamped render, both losses
    and the nine gradient columns against train_grads64; the render
    bit-identical to the op path's."""
    p, r = S.fused_case(cid)
    render, losses, g = _step(p, cuda)
    _check_fused(cid, tile_kernel, render, losses, g)
    m = _model(p, cuda, fused_train=False)
    img = m()["render"]
    assert torch.equal(render, img[0].detach())


@pytest.mark.parametrize("cid", S.FUSED_IDS)
def test_fused_step_deterministic(cuda, cid):
    """torch.use_deterministic_algorithms(True) (the kDet instance): the same
    bars, and two runs bitwise equal."""
    p, r = S.fused_case(cid)
    with deterministic():
        a = _step(p, cuda)
        b = _step(p, cuda)
    _check_fused(cid, "det", *a)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("cid", S.FUSED_IDS)
def test_production_train_iter(cuda, cid):
    """GaussianVideoFrame.train_iter for three steps on one target with
    learning rate 0 (the bound step, carried bins, the tile kernel enqueued
    ahead): adan.h's update leaves p unchanged at lr = 0 and stores neg_pre_grad
    = -g, so every step's gradient is read off the optimizer state and held to
    the same bars; the parameters stay bitwise at their start."""
    p, r = S.fused_case(cid)
    H, W = p["H"], p["W"]
    m = _model(p, cuda, lr=0.0, fused_train=True)
    gt = T(p["gt"]).view(1, 3, H, W)
    names = ["_xyz", "_cholesky", "_features_dc"] + (["rgb_W"] if p["rgbw_train"] else [])
    start = {k: getattr(m, k).detach().clone() for k in names}
    with torch.no_grad():  # the frame render of the same parameters (they never change)
        render = m()["render"][0].clone()
    for it in (1, 2, 3):
        loss, psnr = m.train_iter(gt, it)
        torch.cuda.synchronize()
        cols = [-m.optimizer.state[getattr(m, k)]["neg_pre_grad"] for k in names]
        if not p["rgbw_train"]:
            cols.append(torch.zeros(len(p["xyz"]), 1, device=cuda))
        g = torch.cat(cols, 1)
        # train_iter returns its own loss and the PSNR of the mean squared error
        mse = 10.0 ** (-psnr / 10.0)
        losses = [mse, float(loss)] if p["loss"] == "L1" else [float(loss), r["losses"][1]]
        assert p["loss"] == "L1" or math.isclose(mse, float(loss), rel_tol=1e-12)
        _check_fused(cid, f"train_iter-{it}", render, np.array(losses), g)
        for k in names:
            assert torch.equal(getattr(m, k).detach(), start[k]), (it, k)
    assert m.fused_steps == 3
    assert m._bound_step.tiled_steps >= 1
