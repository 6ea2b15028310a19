"""GPU: the weighted Y/U/V loss in the fused training step (train.hip's band
tile kernel, ``loss_kind`` 2) on the cases of tests/yuv_loss_cases.py: render,
both loss words and the nine gradient columns against the float64 reference
within that file's bars (4 x the float32 restatement's worst, measured on the
CPU), in the atomic and the deterministic instances and through the production
``train_iter`` (the bound step, carried bins, the tile kernel enqueued ahead);
the identity matrix as L2, bit for bit; the compression stage's fused step and
run against the op statement; the refusals.  Every figure is printed before it
is asserted (``YUV-ERR`` lines; pytest -s shows them)."""
import contextlib
import copy
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sum_cases as S
import yuv_loss_cases as Y
from conftest import knobs
from gsvc_amd.knobs import Knob

pytestmark = pytest.mark.gpu


def T(a, dev="cuda"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


@contextlib.contextmanager
def deterministic():
    prev = torch.are_deterministic_algorithms_enabled()
    warn = torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev, warn_only=warn)


def _step(p, dev, loss_type, spec=None):
    """train_step_sum with the test hooks: (render [3, H, W], losses [2],
    grads [N, 9]) as device tensors."""
    from gsvc_amd.train import train_step_sum
    n, H, W = p["xyz"].shape[0], p["H"], p["W"]
    g = torch.empty((n, 9), device=dev)
    render = torch.empty((1, 3, H, W), device=dev)
    losses = train_step_sum(T(p["xyz"]), T(p["chol"]), T(p["feat"]), T(p["rgbw"]), p["rgbw_train"],
                            T(p["bound"]).view(1, 3), T(p["bg"]), T(p["gt"]).view(1, 3, H, W), H, W,
                            loss_type, render_out=render, grads_out=g, yuv_loss=spec)
    return render[0], losses, g


def _check(cid, what, render, losses, g):
    """Print every figure against yuv_reference, then hold each to its bar."""
    p, r, _ = Y.case(cid)
    errs = Y.yuv_errors(cid, N(render), N(losses) if torch.is_tensor(losses) else losses, N(g))
    flat = []
    for k in Y.KEYS:
        v = errs[k]
        if isinstance(v, tuple):
            whole, edge, tile, where = v
            flat += [(k + ".whole", whole, k), (k + ".edge", edge, k), (f"{k}.tile[{where}]", tile, k)]
        else:
            flat.append((k, v, k))
    for name, val, k in flat:
        print(f"YUV-ERR {cid} {what} {name} {val:.3e} bar {Y.BARS[k]:.3e}")
    for name, val, k in flat:
        assert val <= Y.BARS[k], (cid, what, name, val, Y.BARS[k])
    if r["M"] < 1:
        assert not N(g).any()
    assert not N(g)[~r["proj"]["ok"]].any()  # a skipped (det = 0) splat: exactly zero


@pytest.mark.parametrize("cid", Y.IDS)
def test_fused_step_yuv_against_float64(cuda, cid):
    """gsvc_train_step_sum_args with loss_kind 2: the clamped render, the RGB
    mean squared error, the Y/U/V loss and the nine gradient columns against
    the float64 reference; the render bit-identical to the L2 step's."""
    p, r, _ = Y.case(cid)
    render, losses, g = _step(p, cuda, "YUV", Y.spec_of(cid))
    _check(cid, "band", render, losses, g)
    render2, losses2, _ = _step(p, cuda, "L2")
    assert torch.equal(render, render2)
    assert torch.equal(losses[0], losses2[0])  # word 0 is the L2 step's own sum


@pytest.mark.parametrize("cid", Y.IDS)
def test_fused_step_yuv_deterministic(cuda, cid):
    """torch.use_deterministic_algorithms(True) (the kDet instance): the same
    bars, and two runs bitwise equal."""
    p, r, _ = Y.case(cid)
    with deterministic():
        a = _step(p, cuda, "YUV", Y.spec_of(cid))
        b = _step(p, cuda, "YUV", Y.spec_of(cid))
    _check(cid, "det", *a)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("cid", ["counts-420", "17x15-444", "37x45-444"])
def test_identity_matrix_is_l2(cuda, cid):
    """M = I with weights (1, 1, 1) at 4:4:4 is the L2 loss: e = d exactly, w' =
    1 and G's diagonal is float(2 / numel), L2's norm, so the deterministic
    step's gradients are the L2 step's bit for bit; word 1 (three products
    summed per pixel, then added) equals word 0 (a chain of three fmas) to the
    loss's bar."""
    from gsvc_amd.video import YuvFormat, YuvLoss
    p, r, _ = Y.case(cid)
    spec = YuvLoss(YuvFormat(chroma="444"), (1, 1, 1), matrix=np.eye(3))
    with deterministic():
        render, losses, g = _step(p, cuda, "YUV", spec)
        render2, losses2, g2 = _step(p, cuda, "L2")
    assert torch.equal(g, g2) and torch.equal(render, render2)
    assert g.any()
    l0, l1 = (float(x) for x in N(losses))
    print(f"YUV-ERR {cid} identity word1/word0 - 1 = {l1 / l0 - 1:.3e} bar {Y.BARS['yuv_loss_rel']:.3e}")
    assert l0 == float(N(losses2)[0]) and abs(l1 - l0) <= Y.BARS["yuv_loss_rel"] * l0


def _model(p, dev, spec, **kw):
    """A GaussianVideoFrame with loss_type "YUV" holding the case's parameters."""
    from gsvc_amd.frame import make_frame_model
    m = make_frame_model(p["H"], p["W"], p["xyz"].shape[0], dev, seed=0, isremoval=p["rgbw_train"],
                         loss_type="YUV", yuv_loss=spec, **kw)
    with torch.no_grad():
        m._xyz.copy_(T(p["xyz"]))
        m._cholesky.copy_(T(p["chol"]))
        m._features_dc.copy_(T(p["feat"]))
        m.rgb_W.copy_(T(p["rgbw"]))
        m.background.copy_(T(p["bg"]))
    return m


@pytest.mark.parametrize("cid", ["counts-420", "counts-rgbw-420", "span-420", "38x46-420", "37x46-422",
                                 "37x45-444", "empty-420"])
def test_production_train_iter_yuv(cuda, cid):
    """GaussianVideoFrame.train_iter for three steps on one target at learning
    rate 0 (the pattern of test_sum_edges.py::test_production_train_iter):
    adan.h's update stores neg_pre_grad = -g, so every step's gradient is read
    off the optimizer state and held to the bars; the returned loss is the
    Y/U/V loss of the model's own render and the PSNR the RGB one; the op path
    (fused_train=False: autograd through loss_fn) agrees within the bars."""
    from gsvc_amd.frame import yuv_loss
    p, r, _ = Y.case(cid)
    spec = Y.spec_of(cid)
    H, W = p["H"], p["W"]
    gt = T(p["gt"]).view(1, 3, H, W)
    names = ["_xyz", "_cholesky", "_features_dc"] + (["rgb_W"] if p["rgbw_train"] else [])

    def grads_of(m):
        cols = [-m.optimizer.state[getattr(m, k)]["neg_pre_grad"] for k in names]
        if not p["rgbw_train"]:
            cols.append(torch.zeros(len(p["xyz"]), 1, device=cuda))
        return torch.cat(cols, 1)

    m = _model(p, cuda, spec, lr=0.0, fused_train=True)
    start = {k: getattr(m, k).detach().clone() for k in names}
    with torch.no_grad():
        render = m()["render"][0].clone()
        own = float(yuv_loss(render.double(), gt[0].double(), spec))
    for it in (1, 2, 3):
        loss, psnr = m.train_iter(gt, it)
        torch.cuda.synchronize()
        mse = 10.0 ** (-psnr / 10.0)
        _check(cid, f"train_iter-{it}", render, np.array([mse, float(loss)]), grads_of(m))
        assert abs(float(loss) - own) <= Y.BARS["yuv_loss_rel"] * own
        for k in names:
            assert torch.equal(getattr(m, k).detach(), start[k]), (it, k)
    assert m.fused_steps == 3
    assert m._bound_step.tiled_steps >= 1
    # the op path: project -> rasterize -> clamp -> loss_fn("YUV") -> autograd -> Adan
    o = _model(p, cuda, spec, lr=0.0, fused_train=False)
    loss, psnr = o.train_iter(gt, 1)
    torch.cuda.synchronize()
    assert o.fused_steps == 0
    if r["M"] < 1:  # nothing flows: the parameters have no gradient, Adan no state
        assert abs(float(loss) - own) <= Y.BARS["yuv_loss_rel"] * own
        return
    _check(cid, "op-path", render, np.array([10.0 ** (-psnr / 10.0), float(loss)]), grads_of(o))


def test_changed_spec_rebuilds_the_bound_step(cuda):
    from gsvc_amd.frame import yuv_loss
    from gsvc_amd.video import YuvFormat, YuvLoss
    cid = "38x46-420"
    p, r, _ = Y.case(cid)
    gt = T(p["gt"]).view(1, 3, p["H"], p["W"])
    m = _model(p, cuda, Y.spec_of(cid), lr=0.0, fused_train=True)
    with torch.no_grad():
        render = m()["render"]
    m.train_iter(gt, 1)
    first = m._bound_step
    for spec in (YuvLoss(YuvFormat(), (1, 0, 0)), YuvLoss(YuvFormat(chroma="444"), (1, 1, 1))):
        m.yuv_loss = spec
        loss, _ = m.train_iter(gt, 2)
        assert m._bound_step is not first
        want = float(yuv_loss(render.double(), gt.double(), spec))
        assert abs(float(loss) - want) <= Y.BARS["yuv_loss_rel"] * want
    m.loss_type = "L2"
    loss, psnr = m.train_iter(gt, 3)
    assert math.isclose(float(loss), 10.0 ** (-psnr / 10.0), rel_tol=1e-12)


# ---------------------------------------------------------------- the compression stage
QH, QW = 32, 48
QNAMES = ("xyz", "chol", "feat", "scale", "beta")


def _quant_model(n, spec):
    import quant_cases as Q
    m = Q.model_from_case(Q.make_case(n), QH, QW, device="cuda")
    m.loss_type, m.yuv_loss = "YUV", spec
    vq = m.features_dc_quantizer
    with torch.no_grad():  # a codebook state mid-training
        vq.cluster_size.fill_(n / 8 + 1)
        vq.embed_avg.copy_(vq.codebooks * vq.cluster_size[..., None])
    return m.train()


def test_quant_step_yuv(cuda):
    """The compression stage's fused step and a run of 3 on a 48x32
    GaussianVideoFrameQ with loss_type "YUV", against train_iter_quantize (the
    op statement: forward_quantize, loss_fn("YUV") + the VQ term, autograd) from
    equal states, with test_quant_train_gpu.py's comparison for L2: gradients at
    rtol 1e-4 / atol 1e-4 of the tensor's largest, losses at 1e-5, the render
    bit for bit; over the run (a flipped code makes single parameters diverge)
    the per-step PSNR within the project's 0.05 dB (test_quant_train_gpu.py's
    trajectory bar) and the first step's loss at 1e-5.  The logged loss is the
    Y/U/V loss plus the VQ term."""
    from gsvc_amd.frame import loss_fn, synthetic_gt, yuv_loss
    from gsvc_amd.video import YuvFormat, YuvLoss
    n = 65
    spec = YuvLoss(YuvFormat(8, "bt709", True), (6, 1, 1))
    gt = synthetic_gt(QH, QW, 11, cuda)
    m, ref = _quant_model(n, spec), _quant_model(n, spec)
    with torch.no_grad():
        ref.quantized(commit=True)
    pkg = ref.forward_quantize()
    img = pkg["render"]
    loss = loss_fn(img.squeeze(0), gt.squeeze(0), "YUV", lambda_value=0, yuv_loss=spec) + pkg["vq_loss"]
    loss.backward()
    mse = float(F.mse_loss(img.detach(), gt))
    uq = ref.cholesky_quantizer
    want = [p.grad for p in (ref._xyz, ref._cholesky, ref._features_dc, uq.scale, uq.beta)]
    ref.optimizer.zero_grad(set_to_none=True)

    g = torch.empty((8 * n + 6,), device=cuda)
    render = torch.empty((1, 3, QH, QW), device=cuda)
    words = m._fused_step(gt, render_out=render, grads_out=g)
    got = [g[:2 * n], g[2 * n:5 * n], g[5 * n:8 * n], g[8 * n:8 * n + 3], g[8 * n + 3:]]
    for name, a, r in zip(QNAMES, got, want):
        a, r = a.cpu().numpy().reshape(-1), r.cpu().numpy().reshape(-1)
        np.testing.assert_allclose(a, r, rtol=1e-4, atol=1e-4 * float(np.abs(r).max()), err_msg=name)
    assert torch.equal(render, img.detach())
    np.testing.assert_allclose(words[0], mse, rtol=1e-5)
    np.testing.assert_allclose(words[1], float(yuv_loss(img.detach().double(), gt.double(), spec)), rtol=1e-5)
    vq = m.features_dc_quantizer
    vq_term = vq.commitment_weight * (words[2] + words[3]) / (3 * n)
    np.testing.assert_allclose(words[1] + vq_term, float(loss.detach()), rtol=1e-5)
    # the public step from the same state returns that loss and the RGB PSNR
    lf, pf = m.train_iter_quantize_fused(gt)
    assert lf.device.type == "cpu" and lf.shape == ()
    np.testing.assert_allclose(float(lf), float(loss.detach()), rtol=1e-5)
    assert pf == pytest.approx(10 * math.log10(1 / mse), rel=1e-5)
    # a run of 3 from a fresh pair of equal states: the log's loss is word 1 + the
    # VQ term; the first step is the op method's, the trajectory follows it
    m, ref = _quant_model(n, spec), _quant_model(n, spec)
    losses, psnrs = m.train_run_quantize_fused(gt, 3)
    log = np.array(m.__dict__["_bound_quant_step"].run_log[:12], np.float32).reshape(3, 4)
    for i in range(3):
        w = [float(x) for x in log[i]]  # (the words as doubles, as the method adds them)
        assert losses[i] == float(np.float32(w[1] + vq.commitment_weight * (w[2] + w[3]) / (3 * n)))
        assert psnrs[i] == 10 * math.log10(1.0 / w[0])
        assert w[1] != w[0]
        lo, po = ref.train_iter_quantize(gt)
        print(f"YUV-QUANT run step {i}: fused loss {losses[i]:.6e} psnr {psnrs[i]:.4f}; "
              f"op loss {float(lo.detach()):.6e} psnr {po:.4f}")
        assert abs(psnrs[i] - po) <= 0.05
        if i == 0:
            np.testing.assert_allclose(losses[i], float(lo.detach()), rtol=1e-5)
            assert po == pytest.approx(psnrs[i], rel=1e-5)
    assert m.optimizer.param_groups[0]["step"] == ref.optimizer.param_groups[0]["step"] == 3


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_workspace_usable(cuda):
    """Odd H at 4:2:0, a NULL loss_yuv, a zero weight sum and kind 2 under
    Knob.TILE_WG256 = 1: GSVC_ERR_ARG with the reason, nothing launched, and
    the next L2 step on the same workspace is what it was before."""
    from gsvc_amd import _lib
    from gsvc_amd.train import train_step_sum
    from gsvc_amd.video import YuvLoss
    cid = "38x46-420"
    p, r, _ = Y.case(cid)
    before = [x.clone() for x in _step(p, cuda, "L2")]

    def l2_again():
        render, losses, g = _step(p, cuda, "L2")
        assert torch.equal(render, before[0]) and torch.equal(losses, before[1])
        # (float atomics: the gradients repeat to rounding, not to the bit)
        assert float((g - before[2]).abs().max()) <= 1e-5 * float(before[2].abs().max())

    class ZeroWeights:
        chroma_code = 0

        def words(self):
            return (ctypes.c_float * 12)(*YuvLoss().M.reshape(-1).tolist(), 0.0, 0.0, 0.0)

    # a zero weight sum
    with pytest.raises(RuntimeError, match="sum to zero"):
        _step(p, cuda, "YUV", ZeroWeights())
    l2_again()
    # odd H at 4:2:0: the case's parameters on a 37-row frame
    q = dict(p, H=37, gt=p["gt"][:, :37].copy())
    with pytest.raises(RuntimeError, match="does not fit 4:2:0"):
        _step(q, cuda, "YUV", YuvLoss())
    l2_again()
    # kind 2 under the 256-thread diagnostic kernel
    with knobs((Knob.TILE_WG256, 1)):
        with pytest.raises(RuntimeError, match="TILE_WG256"):
            _step(p, cuda, "YUV", Y.spec_of(cid))
        wg = _step(p, cuda, "L2")  # (the diagnostic library's own workspace use)
    assert torch.equal(wg[0], before[0])
    l2_again()
    # a NULL loss_yuv, through the struct
    from gsvc_amd.train import _StepArgs, _raw_stream, _workspace
    n, H, W = p["xyz"].shape[0], p["H"], p["W"]
    t = [T(p[k]) for k in ("xyz", "chol", "feat", "rgbw", "bound", "bg", "gt")]
    ws = _workspace(cuda, n, H, W)
    out = torch.empty(2, device=cuda)
    g = torch.empty((n, 9), device=cuda)
    hp = (ctypes.c_double * 10)()
    a = _StepArgs()
    a.num_points, a.xyz, a.cholesky, a.features, a.rgb_w = n, *(x.data_ptr() for x in t[:4])
    a.cholesky_bound, a.background, a.gt = (x.data_ptr() for x in t[4:])
    a.img_height, a.img_width, a.loss_kind, a.frame_index = H, W, 2, ws.frame
    a.adan_hparams, a.loss, a.grads_out = ctypes.addressof(hp), out.data_ptr(), g.data_ptr()
    a.workspace, a.workspace_bytes, a.stream = ws.buf_ptr, ws.buf.numel(), _raw_stream(cuda.index)
    lib = _lib.load()
    assert lib.gsvc_train_step_sum_args(ctypes.byref(a)) == 1
    assert b"needs loss_yuv" in lib.gsvc_last_error()
    l2_again()
    # and the fused step still runs the loss after all that
    _check(cid, "after-refusals", *_step(p, cuda, "YUV", Y.spec_of(cid)))
