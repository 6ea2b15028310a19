"""GPU: the fused quantized training step (csrc/quant_train.hip,
``gsvc_quant_train_step`` / ``gsvc_quant_adan_step``,
``train_iter_quantize_fused``).

The quantizer half on its own against the sequence of existing ops
(gsvc_quant_params_backward, ops.adan_step, ResidualVQ8.ema_update) on copies:
parameters and Adan state bit for bit, the codebooks' moving average against
the float64 restatement of tests/quant_train_cases.py; the whole step against
autograd through forward_quantize from equal states; the hand-off between the
two training methods; bitwise reproducibility; a 20-step trajectory."""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import quant_cases as Q
import quant_train_cases as QT
from gsvc_amd import compress as C
from gsvc_amd import ops
from gsvc_amd import quantize as QZ

pytestmark = pytest.mark.gpu

H, W = 40, 72  # partial tiles on both axes, 15 tiles
HALF_CASES = ([(n, d, t) for n in QT.SIZES for d in (False, True) for t in (1, 2)]
              + [(QT.BIG, False, 2)])
_STATE = ("exp_avg", "exp_avg_sq", "exp_avg_diff", "neg_pre_grad")
NAMES = ("xyz", "chol", "feat", "scale", "beta")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    """The tensor's bit patterns (NaNs compare by their bits)."""
    return t.detach().contiguous().cpu().view(torch.int32).numpy()


def same(a, b, name=""):
    """Equal bits, a NaN matching any NaN (its sign and payload carry nothing)."""
    a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=name)
    keep = ~np.isnan(a)
    np.testing.assert_array_equal(a[keep].view(np.int32), b[keep].view(np.int32), err_msg=name)


def _device_inputs(h):
    case = h["case"]
    params = [T(case[k]) for k in NAMES]
    tables = [T(case["cb"]), T(h["cluster"]), T(h["embed"])]
    state = [T(s) for per in h["state"] for s in per]
    prev = None if case["prev"] is None else tuple(T(p) for p in case["prev"])
    # the forward's codes and commitment sums (gsvc_quant_params_forward)
    _, _, _, _, codes, sums = QZ._forward_hip(*params, tables[0], T(case["bound"]), prev, True)
    return params, tables, state, T(h["rec"]), codes, sums


def _op_sequence(h):
    """gsvc_quant_params_backward, ops.adan_step over the five tensors, then
    ResidualVQ8.ema_update (on the pre-update features), on their own copies."""
    params, tables, state, rec, codes, _ = _device_inputs(h)
    n, t = h["n"], h["t"]
    xyz, chol, feat, scale, beta = params
    vc = T(np.full(2, np.float32(QT.COMMIT_WEIGHT / (3.0 * n)), np.float32))
    grads = QZ._backward_hip(chol, feat, scale, beta, tables[0], codes, rec[:, 0:2].contiguous(),
                             rec[:, 2:5].contiguous(), rec[:, 5:8].contiguous(), vc)
    feat_pre = feat.clone()
    cols = [[state[4 * q + k] for q in range(5)] for k in range(4)]
    if t == 1:  # Adan.step's first step: neg_pre_grad = grad * -clip
        for q in range(5):
            cols[3][q].copy_(grads[q].mul(-1.0))
    hp = QT.hparams(t)
    ops.adan_step(params, list(grads), *cols, beta1=hp[0], beta2=hp[1], beta3=hp[2],
                  bias_correction1=hp[3], bias_correction2=hp[4], bias_correction3_sqrt=hp[5], lr=hp[6],
                  weight_decay=hp[7], eps=hp[8], no_prox=False, clip_global_grad_norm=1.0)
    vq = QZ.ResidualVQ8(decay=QT.DECAY, eps=QT.EPS).cuda()
    vq.codebooks.copy_(tables[0])
    vq.cluster_size.copy_(tables[1])
    vq.embed_avg.copy_(tables[2])
    vq.ema_update(feat_pre, codes)
    torch.cuda.synchronize()
    return dict(params=params, state=state, grads=grads,
                tables=[vq.codebooks, vq.cluster_size, vq.embed_avg], codes=codes)


def _fused_half(h, grads_out=None):
    params, tables, state, rec, codes, sums = _device_inputs(h)
    loss = torch.full((4,), -1.0, device="cuda")
    QT.quant_adan_step(torch.device("cuda:0"), params, tables, state, rec, codes, sums, h["t"],
                       first=h["t"] == 1, grads_out=grads_out, loss=loss)
    return dict(params=params, state=state, tables=tables, loss=loss, sums=sums)


@pytest.fixture(scope="module")
def refs(cuda):
    """Per case the op sequence's results and the float64 restatement, and the
    bar for embed_avg / codebooks: 4 x the worst error of the fp32 torch
    ema_update against the restatement over these same cases (the bar comes
    from the reference, never from the kernel)."""
    out, worst = {}, {"embed_avg": 0.0, "codebooks": 0.0}
    for n, delta, t in HALF_CASES:
        h = QT.half_case(n, delta, t)
        seq = _op_sequence(h)
        case = h["case"]
        r64 = QT.ema_ref64(case["feat"], seq["codes"].cpu().numpy(), case["cb"], h["cluster"], h["embed"])
        worst["embed_avg"] = max(worst["embed_avg"], QT.rel_err(seq["tables"][2].cpu().numpy(),
                                                                r64["embed_avg"]))
        worst["codebooks"] = max(worst["codebooks"], QT.rel_err(seq["tables"][0].cpu().numpy(),
                                                                r64["codebooks"]))
        out[(n, delta, t)] = (h, seq, r64)
    bar = {k: 4 * v for k, v in worst.items()}
    print("torch ema_update fp32 vs float64, worst over the cases:", worst, "-> bar", bar)
    assert all(v > 0 for v in bar.values())
    return out, bar


@pytest.mark.parametrize("n,delta,t", HALF_CASES)
def test_half_matches_the_op_sequence(refs, n, delta, t):
    cases, bar = refs
    h, seq, r64 = cases[(n, delta, t)]
    got = _fused_half(h)
    for q, name in enumerate(NAMES):
        np.testing.assert_array_equal(bits(got["params"][q]), bits(seq["params"][q]), err_msg=name)
        for k in range(4):
            np.testing.assert_array_equal(bits(got["state"][4 * q + k]), bits(seq["state"][4 * q + k]),
                                          err_msg=f"{name}.{_STATE[k]}")
    cb, cs, em = (x.cpu().numpy() for x in got["tables"])
    np.testing.assert_array_equal(cs, QT.cluster_size_f32(h["cluster"], r64["counts"]))
    e_em, e_cb = QT.rel_err(em, r64["embed_avg"]), QT.rel_err(cb, r64["codebooks"])
    print(f"N={n} delta={delta} t={t}: embed_avg {e_em:.3e} (bar {bar['embed_avg']:.3e}) "
          f"codebooks {e_cb:.3e} (bar {bar['codebooks']:.3e})")
    assert e_em <= bar["embed_avg"] and e_cb <= bar["codebooks"]
    # the loss words of the half alone: no render, the given commitment sums
    loss = got["loss"].cpu().numpy()
    np.testing.assert_array_equal(loss[:2], [0, 0])
    np.testing.assert_array_equal(loss[2:], got["sums"].cpu().numpy())
    # equal inputs, equal bits in every output
    again = _fused_half(h)
    for a, b in zip(got["params"] + got["state"] + got["tables"] + [got["loss"]],
                    again["params"] + again["state"] + again["tables"] + [again["loss"]]):
        np.testing.assert_array_equal(bits(a), bits(b))


def test_half_nan_cholesky_gives_what_the_op_sequence_gives(cuda):
    h = QT.half_case(65, False, 2)
    h["case"] = dict(h["case"])
    h["case"]["chol"] = h["case"]["chol"].copy()
    h["case"]["chol"][2, 1] = np.nan
    seq, got = _op_sequence(h), _fused_half(h)
    assert np.isnan(seq["params"][3].cpu().numpy()[1])  # v_scale[1] is NaN, and so scale[1]
    assert np.isfinite(seq["params"][1].cpu().numpy()[np.arange(65) != 2]).all()
    for q, name in enumerate(NAMES):
        same(got["params"][q], seq["params"][q], name)
        for k in range(4):
            same(got["state"][4 * q + k], seq["state"][4 * q + k], f"{name}.{_STATE[k]}")
    for a, b in zip(got["tables"], seq["tables"]):  # the colours' tables are untouched by it
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())


@pytest.mark.parametrize("n", [65, 4099])
def test_half_hook_writes_gradients_and_changes_nothing(cuda, n):
    h = QT.half_case(n, True, 2)
    before = _device_inputs(h)
    seq = _op_sequence(h)
    g = torch.full((8 * n + 6,), 7.0, device="cuda")
    got = _fused_half(h, grads_out=g)
    for a, b in zip(got["params"] + got["state"] + got["tables"], before[0] + before[2] + before[1]):
        np.testing.assert_array_equal(bits(a), bits(b))
    want = torch.cat([x.reshape(-1) for x in seq["grads"]])
    np.testing.assert_array_equal(bits(g), bits(want))


# --------------------------------------------------------------------------
# the whole step from equal states

def _case_model(n, delta, loss_type):
    case = Q.make_case(n, delta=delta)
    m = Q.model_from_case(case, H, W, device="cuda")
    m.loss_type = loss_type
    vq = m.features_dc_quantizer
    with torch.no_grad():  # a codebook state mid-training
        vq.cluster_size.fill_(n / 8 + 1)
        vq.embed_avg.copy_(vq.codebooks * vq.cluster_size[..., None])
    return m.train()


@pytest.mark.parametrize("loss_type", ["L2", "L1"])
@pytest.mark.parametrize("delta", [False, True])
@pytest.mark.parametrize("n", [1, 65, 300])
def test_whole_step_matches_autograd(cuda, n, delta, loss_type):
    from gsvc_amd.frame import loss_fn, synthetic_gt
    m = _case_model(n, delta, loss_type)
    gt = synthetic_gt(H, W, 11, cuda)
    ref = copy.deepcopy(m)
    with torch.no_grad():
        sums = ref.quantized(commit=True)[5]
    pkg = ref.forward_quantize()
    img = pkg["render"]
    loss = loss_fn(img.squeeze(0), gt.squeeze(0), loss_type, lambda_value=0) + pkg["vq_loss"]
    loss.backward()
    mse = float(F.mse_loss(img.detach(), gt))
    uq = ref.cholesky_quantizer
    want = [p.grad for p in (ref._xyz, ref._cholesky, ref._features_dc, uq.scale, uq.beta)]

    before = {k: v.clone() for k, v in m.state_dict().items()}
    g = torch.empty((8 * n + 6,), device=cuda)
    render = torch.empty((1, 3, H, W), device=cuda)
    words = m._fused_step(gt, render_out=render, grads_out=g)
    # the hook updates nothing and moves no counter
    for k, v in m.state_dict().items():
        np.testing.assert_array_equal(bits(v.float()), bits(before[k].float()), err_msg=k)
    assert len(m.optimizer.state) == 0 and m.optimizer.param_groups[0].get("step", 0) == 0
    got = [g[:2 * n], g[2 * n:5 * n], g[5 * n:8 * n], g[8 * n:8 * n + 3], g[8 * n + 3:]]
    for name, a, r in zip(NAMES, got, want):
        a, r = a.cpu().numpy().reshape(-1), r.cpu().numpy().reshape(-1)
        np.testing.assert_allclose(a, r, rtol=1e-4, atol=1e-4 * float(np.abs(r).max()), err_msg=name)
    assert torch.equal(render, img.detach())
    np.testing.assert_array_equal(np.array(words[2:], np.float32), sums.cpu().numpy())
    np.testing.assert_allclose(words[0], mse, rtol=1e-5)
    vq = m.features_dc_quantizer
    fused_loss = words[1 if loss_type == "L1" else 0] + vq.commitment_weight * (words[2] + words[3]) / (3 * n)
    np.testing.assert_allclose(fused_loss, float(loss.detach()), rtol=1e-5)
    assert 10 * math.log10(1 / words[0]) == pytest.approx(10 * math.log10(1 / mse), rel=1e-5)
    # and the public method returns these: loss as a host scalar tensor, PSNR from the MSE
    l2, psnr = m.train_iter_quantize_fused(gt)
    assert l2.device.type == "cpu" and l2.shape == ()
    np.testing.assert_allclose(float(l2), float(loss.detach()), rtol=1e-5)
    assert psnr == pytest.approx(10 * math.log10(1 / mse), rel=1e-5)


# --------------------------------------------------------------------------
# hand-off, reproducibility, trajectory

def _fresh_model(n, seed, lr=1e-2, delta=False, loss_type="L2"):
    torch.manual_seed(seed)
    cls = C.GaussianVideoDelta if delta else C.GaussianVideoFrameQ
    m = cls(loss_type=loss_type, opt_type="adan", num_points=n, H=H, W=W, BLOCK_H=16, BLOCK_W=16,
            device="cuda", lr=lr, quantize=True).cuda()
    with torch.no_grad():
        m._cholesky.mul_(3.0)
    m._init_data()
    return m.train()


def _finite(m):
    return all(bool(torch.isfinite(v.float()).all()) for v in m.state_dict().values())


def test_hand_off_between_the_two_methods(cuda):
    from gsvc_amd.frame import synthetic_gt
    gt = synthetic_gt(H, W, 4, cuda)
    m = _fresh_model(65, 1)
    for _ in range(2):
        loss, psnr = m.train_iter_quantize_fused(gt)
        assert math.isfinite(float(loss)) and math.isfinite(psnr)
    opt = m.optimizer
    uq = m.cholesky_quantizer
    for p in (m._xyz, m._cholesky, m._features_dc, uq.scale, uq.beta):
        assert sorted(opt.state[p]) == sorted(_STATE)
        assert all(opt.state[p][k].shape == p.shape for k in _STATE)
    assert opt.param_groups[0]["step"] == 2 and m.scheduler.last_epoch == 2
    _, p_op = m.train_iter_quantize(gt)
    _, p_fused = m.train_iter_quantize_fused(gt)
    assert opt.param_groups[0]["step"] == 4 and m.scheduler.last_epoch == 4
    assert math.isfinite(p_op) and math.isfinite(p_fused) and _finite(m)
    m.load_state_dict(copy.deepcopy(m.state_dict()))
    opt.load_state_dict(copy.deepcopy(opt.state_dict()))
    _, p_again = m.train_iter_quantize_fused(gt)
    assert math.isfinite(p_again) and _finite(m) and opt.param_groups[0]["step"] == 5


def test_compress_video_fused_round_trip(cuda):
    """test_compress_video_round_trip's three tiny frames (a key frame and two
    deltas, the second with fewer splats) with every iteration fused: the
    decoded GOP reproduces the logged PSNR exactly."""
    from gsvc_amd.frame import synthetic_gt
    torch.manual_seed(3)
    frames = [synthetic_gt(H, W, s, "cuda") for s in (1, 2, 3)]
    sd = {}
    for i, n in enumerate((65, 65, 40)):
        sd[f"frame_{i + 1}"] = {"_xyz": torch.atanh(2 * (torch.rand(n, 2) - 0.5)).cuda(),
                                "_cholesky": (3 * torch.rand(n, 3)).cuda(),
                                "_features_dc": torch.rand(n, 3).cuda()}
    out = C.compress_video(sd, frames, K_frames=[1], iterations=3, lr=1e-2, device="cuda",
                           delta_base="decoded", seed=0, fused=True)
    assert [len(s) for s in out["streams"]] == [256 + 7 * 65, 256 + 7 * 65, 256 + 7 * 40]
    assert [C.parse_header(s)["delta"] for s in out["streams"]] == [False, True, True]
    imgs = C.decode_frames(out["streams"], "cuda")
    for f in range(3):
        mse = F.mse_loss(imgs[f:f + 1], frames[f]).item()
        assert 10 * math.log10(1.0 / mse) == out["psnr"][f], f


@pytest.fixture
def deterministic():
    prev = torch.are_deterministic_algorithms_enabled()
    prev_warn = torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    yield
    torch.use_deterministic_algorithms(prev, warn_only=prev_warn)


def test_fused_runs_are_bitwise_reproducible(cuda, deterministic):
    """Everything the step adds has a fixed order; with the render step's
    deterministic backward (at 40x72 a splat touches at most 15 tiles, inside
    the 16 slots per splat train.py allots) two runs of 10 steps from equal
    seeds end in equal bits."""
    from gsvc_amd.frame import synthetic_gt
    gt = synthetic_gt(H, W, 6, cuda)
    runs = []
    for _ in range(2):
        m = _fresh_model(65, 21)
        psnrs = [m.train_iter_quantize_fused(gt)[1] for _ in range(10)]
        opt, uq = m.optimizer, m.cholesky_quantizer
        st = [opt.state[p][k] for p in (m._xyz, m._cholesky, m._features_dc, uq.scale, uq.beta)
              for k in _STATE]
        runs.append(([bits(v.float()) for v in m.state_dict().values()], [bits(s) for s in st],
                     bits(m.features_dc_quantizer.codebooks), C.encode_frame(m.eval()), psnrs))
    a, b = runs
    for x, y in zip(a[0] + a[1] + [a[2]], b[0] + b[1] + [b[2]]):
        np.testing.assert_array_equal(x, y)
    assert a[3] == b[3] and a[4] == b[4]


def test_trajectory_follows_the_op_by_op_method(cuda):
    """20 steps at 40x72 / 300 splats, lr 1e-2, from equal seeds.  A flipped code
    makes single parameters diverge, so the per-step PSNR is compared; the bar
    is the larger of 0.05 dB (the project's video-level bar) and 4 x the largest
    per-step PSNR spread among three runs of the op-by-op method -- taken from
    those runs, not from the fused one."""
    from gsvc_amd.frame import synthetic_gt
    gt = synthetic_gt(H, W, 9, cuda)

    def run(fused):
        m = _fresh_model(300, 33)
        it = m.train_iter_quantize_fused if fused else m.train_iter_quantize
        return np.array([it(gt)[1] for _ in range(20)])

    op = np.stack([run(False) for _ in range(3)])
    spread = float((op.max(0) - op.min(0)).max())
    bar = max(0.05, 4 * spread)
    fused = run(True)
    diff = float(np.abs(fused[None] - op).max())
    print(f"op-by-op PSNR spread over 3 runs {spread:.3e} dB -> bar {bar:.3e} dB; fused vs op-by-op "
          f"{diff:.3e} dB; fused PSNR {fused[0]:.3f} -> {fused[-1]:.3f}")
    assert diff <= bar
    assert fused[-1] >= fused[0]
