"""The weighted Y/U/V training loss without a GPU: the spec (gsvc_amd.video.
YuvLoss), the op path's torch statement (gsvc_amd.frame.yuv_plane_mse /
yuv_loss) against the definition in numpy float64, its tie to the integer
output conversion, the argument structs and the entries' argument checks, and
the premises of tests/yuv_loss_cases.py: the two float64 statements of the
fused step's loss gradient agree, the kernel's folding equals the definition,
every case keeps its decision margins, and the bars are what the float32
restatement measures."""
import ctypes

import numpy as np
import pytest
import torch

import sum_cases as S
import yuv_loss_cases as Y
from gsvc_amd.frame import loss_fn, yuv_loss, yuv_plane_mse
from gsvc_amd.video import YuvFormat, YuvLoss, rgb_to_i420


# ---------------------------------------------------------------- the spec
@pytest.mark.parametrize("fmt", [YuvFormat(), YuvFormat(10, "bt709", True)], ids=str)
def test_matrix_is_the_conversion_table(fmt):
    M = YuvLoss(fmt).M
    assert M.dtype == np.float64 and M.shape == (3, 3)
    assert np.array_equal(M, np.array(fmt.conversion_table()[9:18], np.float64).reshape(3, 3) / 2 ** 20)
    # the cases' own restatement of the table
    assert np.array_equal(M, Y.matrix_of(fmt.bit_depth, fmt.matrix, fmt.full_range))
    # rows: Y sums to the luma span, U and V to zero, up to the table's rounding
    # (the legacy triple: OpenCV's three decimals)
    span = 1.0 if fmt.full_range else 219.0 * 2 ** (fmt.bit_depth - 8) / fmt.peak
    tol = 1e-3 if fmt.is_legacy else 3 / 2 ** 20
    assert abs(M[0].sum() - span) < tol and np.abs(M[1:].sum(1)).max() < tol


def test_spec_defaults_and_reexport():
    import gsvc_amd
    assert gsvc_amd.YuvLoss is YuvLoss
    s = YuvLoss()
    assert s.fmt == YuvFormat() and s.weights == (6.0, 1.0, 1.0) and s.matrix is None and s.chroma_code == 0
    assert YuvLoss(YuvFormat(chroma="422")).chroma_code == 1 and YuvLoss(YuvFormat(chroma="444")).chroma_code == 2
    # the legacy triple keeps OpenCV's constants in any chroma, layout does not matter
    assert np.array_equal(YuvLoss(YuvFormat(chroma="444", layout="semi")).M, s.M)
    eye = YuvLoss(matrix=np.eye(3), weights=(1, 1, 1))
    assert np.array_equal(eye.M, np.eye(3)) and hash(eye) == hash(YuvLoss(matrix=np.eye(3), weights=(1, 1, 1)))
    with pytest.raises(dataclasses_error()):
        s.weights = (1.0, 1.0, 1.0)
    assert list(s.words()) == [np.float32(x) for x in list(s.M.reshape(-1)) + [6.0, 1.0, 1.0]]


def dataclasses_error():
    import dataclasses
    return dataclasses.FrozenInstanceError


@pytest.mark.parametrize("w", [(0, 0, 0), (-1, 2, 2), (1, 1), (1, float("nan"), 1), (float("inf"), 1, 1)],
                         ids=str)
def test_bad_weights_raise(w):
    with pytest.raises(ValueError, match="weights"):
        YuvLoss(weights=w)


def test_bad_matrix_raises():
    with pytest.raises(ValueError, match="3x3"):
        YuvLoss(matrix=np.ones((3, 2)))


# ---------------------------------------------------------------- the torch statement
def _pair(H, W, seed):
    rng = np.random.default_rng(seed)
    return rng.random((3, H, W)), rng.random((3, H, W))


@pytest.mark.parametrize("chroma,H,W", [("420", 6, 10), ("422", 7, 10), ("444", 7, 9)])
def test_torch_statement_against_numpy_float64(chroma, H, W):
    spec = YuvLoss(YuvFormat(10, "bt709", False, chroma), (6.0, 1.0, 2.0))
    ref_spec = dict(M=spec.M, w=np.array(spec.weights), chroma=spec.chroma_code)
    x, t = _pair(H, W, 3)
    mse, L, g = Y.yuv_definition(x, t, ref_spec)
    pred = torch.tensor(x, requires_grad=True)
    planes = yuv_plane_mse(pred, torch.tensor(t), spec)
    assert planes.dtype == torch.float64 and planes.shape == (3,)
    np.testing.assert_allclose(planes.detach().numpy(), mse, rtol=1e-12, atol=0)
    loss = yuv_loss(pred, torch.tensor(t), spec)
    assert abs(loss.item() - L) <= 1e-12 * L
    loss.backward()
    # the closed form: 2 / (H W sum w) sum_k w_k M[k][c] mean_k(B_k(p))
    np.testing.assert_allclose(pred.grad.numpy(), g, rtol=0, atol=1e-12 * np.abs(g).max())
    # [1, 3, H, W] inputs, and the dispatch of loss_fn (float32 there)
    l4 = yuv_loss(torch.tensor(x)[None], torch.tensor(t)[None], spec)
    assert l4.item() == loss.item()
    lf = loss_fn(torch.tensor(x), torch.tensor(t), "YUV", yuv_loss=spec)
    assert lf.dtype == torch.float32 and abs(lf.item() - L) <= 1e-5 * L


def test_loss_fn_default_spec_and_sizes():
    x, t = _pair(4, 6, 5)
    a = loss_fn(torch.tensor(x), torch.tensor(t), "YUV")
    b = loss_fn(torch.tensor(x), torch.tensor(t), "YUV", lambda_value=0.1, yuv_loss=YuvLoss())
    assert a.item() == b.item()
    with pytest.raises(ValueError, match="4:2:0"):
        yuv_loss(torch.rand(3, 5, 6), torch.rand(3, 5, 6))
    with pytest.raises(ValueError, match="4:2:2"):
        yuv_loss(torch.rand(3, 5, 7), torch.rand(3, 5, 7), YuvLoss(YuvFormat(chroma="422")))
    yuv_loss(torch.rand(3, 5, 7), torch.rand(3, 5, 7), YuvLoss(YuvFormat(chroma="444")))


@pytest.mark.parametrize("name", ["yuv420p", "yuv422p10le", "yuv444p"])
def test_tie_to_the_integer_conversion(name):
    """Per plane |sqrt(sse_k / samples_k) - peak sqrt(mse_k)| <= 2 codes: each
    side's code differs from the unrounded value by under one code (0.5 from the
    final rounding, 0.5 sum_c |M[k][c]| <= 0.5 from the RGB quantisation), so the
    two difference vectors differ by under 2 per sample, and so do their
    root-mean-square norms (the triangle inequality)."""
    f = YuvFormat.from_pix_fmt(name)
    H, W = 36, 44
    g = torch.Generator().manual_seed(11)
    t = torch.rand(3, H, W, generator=g)
    p = (t + 0.1 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    ref = rgb_to_i420(t, fmt=f)
    _, sse = rgb_to_i420(p, ref=ref, fmt=f)
    ch, cw = f.chroma_shape(H, W)
    samples = np.array([H * W, ch * cw, ch * cw], np.float64)
    mse = yuv_plane_mse(p.double(), t.double(), YuvLoss(f)).numpy()
    got = np.sqrt(sse[0].numpy().astype(np.float64) / samples)
    want = f.peak * np.sqrt(mse)
    print("YUV-TIE", name, got, want)
    assert (want > 5).all()  # the noise is well above the rounding
    assert (np.abs(got - want) <= 2.0).all(), (got, want)


# ---------------------------------------------------------------- structs and entries
def test_structs_carry_the_two_fields_last():
    from gsvc_amd.compress import _QuantStepArgs
    from gsvc_amd.train import LOSS_KIND, _StepArgs
    assert LOSS_KIND == {"L2": 0, "L1": 1, "YUV": 2}
    for cls in (_StepArgs, _QuantStepArgs):
        assert [f[0] for f in cls._fields_[-2:]] == ["loss_yuv", "loss_chroma"]
        assert cls._fields_[-2][1] is ctypes.c_void_p and cls._fields_[-1][1] is ctypes.c_int


def test_train_step_sum_admits_the_kind():
    from gsvc_amd.train import train_step_sum
    z = torch.zeros
    args = (z(4, 2), z(4, 3), z(4, 3), None, False, z(1, 3), z(3), z(1, 3, 4, 4), 4, 4)
    with pytest.raises(ValueError, match="not 'SSIM'"):
        train_step_sum(*args, "SSIM")
    # "YUV" gets past the kind's check to the tensors' (CPU tensors here)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        train_step_sum(*args, "YUV", yuv_loss=YuvLoss())
    with pytest.raises(TypeError):  # keyword-only, after the existing positionals
        train_step_sum(*args, "YUV", (), (), 0, None, None, YuvLoss())


def _dummy_step_args(H=40, W=72):
    """A gsvc_train_step_args that passes the checks before the loss's: the
    pointers are never dereferenced, a failing check returns first."""
    from gsvc_amd import _lib
    from gsvc_amd.train import _StepArgs
    lib = _lib.load()
    d = 16
    hp = (ctypes.c_double * 10)()
    a = _StepArgs()
    a.num_points, a.xyz, a.cholesky, a.features, a.background, a.gt, a.loss = 10, d, d, d, d, d, d
    a.img_height, a.img_width, a.loss_kind, a.adan_hparams = H, W, 2, ctypes.addressof(hp)
    return lib, a, hp


REFUSALS = [
    # (size, the twelve words or None, chroma code, part of the message)
    ((40, 72), None, 0, b"needs loss_yuv"),
    ((40, 72), "ok", 3, b"loss_chroma"),
    ((40, 72), "ok", -1, b"loss_chroma"),
    ((41, 72), "ok", 0, b"does not fit 4:2:0"),
    ((40, 71), "ok", 0, b"does not fit 4:2:0"),
    ((40, 71), "ok", 1, b"does not fit 4:2:2"),
    ((40, 72), [0.0, 0.0, 0.0], 0, b"sum to zero"),
    ((40, 72), [6.0, -1.0, 1.0], 0, b"negative loss weight"),
    ((40, 72), [6.0, float("nan"), 1.0], 0, b"not finite"),
    ((40, 72), [float("inf"), 1.0, 1.0], 0, b"not finite"),
]


@pytest.mark.parametrize("size,words,chroma,msg", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_entries_refuse_without_launch(size, words, chroma, msg):
    """Kind 2's argument errors, from both entries, before anything is launched."""
    lib, a, hp = _dummy_step_args(*size)
    buf = None
    if words is not None:
        w = [6.0, 1.0, 1.0] if words == "ok" else words
        buf = (ctypes.c_float * 12)(*YuvLoss().M.reshape(-1).tolist(), *w)
        a.loss_yuv = ctypes.addressof(buf)
    a.loss_chroma = chroma
    assert lib.gsvc_train_step_sum_args(ctypes.byref(a)) == 1
    assert msg in lib.gsvc_last_error(), lib.gsvc_last_error()
    import test_quant_train_cpu as Q
    lib, q, keep = Q._dummy_args()
    q.img_height, q.img_width, q.loss_kind, q.loss_chroma = size[0], size[1], 2, chroma
    q.train_workspace_bytes = lib.gsvc_train_step_workspace_bytes(10, *size)
    if buf is not None:
        q.loss_yuv = ctypes.addressof(buf)
    assert lib.gsvc_quant_train_step(ctypes.byref(q)) == 1
    assert msg in lib.gsvc_last_error(), lib.gsvc_last_error()


def test_odd_height_fits_422_and_any_size_444():
    """4:2:2 takes an odd height and 4:4:4 any size: the loss's check passes and
    the next one (the workspace's) answers."""
    for size, chroma in (((41, 72), 1), ((41, 71), 2)):
        lib, a, hp = _dummy_step_args(*size)
        buf = YuvLoss().words()
        a.loss_yuv, a.loss_chroma, a.grads_out = ctypes.addressof(buf), chroma, 16
        assert lib.gsvc_train_step_sum_args(ctypes.byref(a)) == 2
        assert b"workspace" in lib.gsvc_last_error()


def test_positional_entry_keeps_two_kinds():
    from gsvc_amd import _lib
    lib = _lib.load()
    d = ctypes.c_void_p(16)
    hp = (ctypes.c_double * 10)()
    rc = lib.gsvc_train_step_sum(10, d, d, None, d, None, 0, d, d, 40, 72, 2, 0, None, hp, 0, d, None, None,
                                 None, ctypes.c_size_t(0), None)
    assert rc == 1 and b"0 (L2) or 1 (L1)" in lib.gsvc_last_error()


def test_models_take_the_spec():
    from gsvc_amd.compress import GaussianVideoFrameQ
    from gsvc_amd.frame import make_frame_model
    spec = YuvLoss(YuvFormat(chroma="422"), (1, 1, 1))
    m = make_frame_model(17, 32, 8, "cpu", seed=0, loss_type="YUV", yuv_loss=spec, fused_render=False)
    assert m.loss_type == "YUV" and m.yuv_loss is spec
    assert make_frame_model(16, 32, 8, "cpu", seed=0, loss_type="YUV").yuv_loss == YuvLoss()
    with pytest.raises(ValueError, match="4:2:0"):
        make_frame_model(17, 32, 8, "cpu", seed=0, loss_type="YUV")
    q = GaussianVideoFrameQ(loss_type="YUV", yuv_loss=spec, num_points=8, H=17, W=32, BLOCK_H=16, BLOCK_W=16,
                            device="cpu", lr=1e-3, quantize=True, opt_type="adan")
    assert q.yuv_loss is spec
    # the op path on the CPU reports the loss of its own render
    gt = torch.rand(1, 3, 17, 32)
    with torch.no_grad():
        want = float(yuv_loss(m()["render"], gt, spec))
    loss, psnr = m.train_iter(gt, 1)
    assert abs(loss.item() - want) <= 1e-6 * want and m.fused_steps == 0


def test_command_lines_take_the_loss():
    from gsvc_amd.video import parse_args
    a = parse_args(["--loss_type", "YUV", "--loss_weights", "4,1,1", "--matrix", "bt709", "--pix_fmt",
                    "yuv422p10le"])
    assert a.yuv_loss == YuvLoss(YuvFormat(10, "bt709", False, "422"), (4.0, 1.0, 1.0))
    assert parse_args(["--loss_type", "YUV"]).yuv_loss == YuvLoss()
    assert parse_args([]).yuv_loss is None
    with pytest.raises(SystemExit):
        parse_args(["--loss_type", "YUV", "--loss_weights", "1,2"])
    with pytest.raises(SystemExit):
        parse_args(["--loss_weights", "1,2,3"])


# ---------------------------------------------------------------- the cases' premises
@pytest.mark.parametrize("cid", Y.IDS)
def test_case_margins_and_statements(cid):
    """The case keeps S.MARGIN_FLOOR in float64; the definition through
    raster_bwd_np and the projection VJP, torch autograd of the same forward,
    and the kernel's folding in float64 give one loss and one gradient."""
    p, r, spec = Y.case(cid)
    for k, floor in S.MARGIN_FLOOR.items():
        assert r["margins"][k] >= floor, (cid, k, r["margins"][k])
    fmt = Y.CASES[cid][1]
    YuvFormat(*fmt).check_size(p["H"], p["W"])
    ref = Y.yuv_reference(cid)
    scale = np.abs(ref["grads"]).max() or 1.0
    img, L, g = Y.yuv_autograd(cid)
    assert np.abs(img - ref["render"]).max() <= 1e-12
    assert abs(L - ref["loss"]) <= 1e-12 * ref["loss"]
    assert np.abs(g - ref["grads"]).max() <= 1e-11 * scale
    _, (mse, Lf), gf = Y.yuv_folded(cid)
    assert mse == ref["mse"] and abs(Lf - ref["loss"]) <= 1e-12 * ref["loss"]
    assert np.abs(gf - ref["grads"]).max() <= 1e-12 * scale
    if r["M"] < 1:
        assert not ref["grads"].any() and ref["loss"] > 0
    else:  # the clamp decides somewhere, and the gradient is not L2's
        assert ref["grads"].any()
        assert np.abs(ref["grads"] - r["grads"]).max() > 1e-3 * scale
    # the spec handed to the code under test is the case's
    s = Y.spec_of(cid)
    assert np.array_equal(s.M, spec["M"]) and s.weights == tuple(spec["w"]) and s.chroma_code == spec["chroma"]


def test_cases_cover_what_they_claim():
    shapes = {(Y.case(c)[0]["H"], Y.case(c)[0]["W"]): Y.CASES[c][1][3] for c in Y.IDS}
    for hw in ((2, 2), (2, 38), (38, 2), (18, 16), (34, 18), (38, 46), (58, 74)):
        assert shapes[hw] == "420"
    assert shapes[(37, 46)] == "422"
    for hw in ((1, 1), (17, 15), (37, 45)):
        assert shapes[hw] == "444"
    fmts = {Y.CASES[c][1][:3] for c in Y.IDS}
    assert {(8, "bt601", False), (8, "bt709", True)} <= fmts and any(f[0] == 10 for f in fmts)
    assert {Y.CASES[c][2] for c in Y.IDS} == {(6.0, 1.0, 1.0), (1.0, 1.0, 1.0), (1.0, 0.0, 0.0)}
    assert Y.case("counts-rgbw-420")[0]["rgbw_train"] and Y.case("empty-420")[1]["M"] < 1
    # blocks that are partly clamped: some 2x2 block of `counts` has 1..3 of its
    # four pixels outside the clamp's pass region in some channel
    pas = Y.case("counts-420")[1]["passes"]
    blocks = pas.reshape(29, 2, 37, 2, 3).sum(axis=(1, 3))
    assert ((blocks > 0) & (blocks < 4)).any()


def test_bars_are_the_float32_restatement():
    """BARS = 4 x WORST, and WORST is what the float32 restatement with
    sequential sums measures on these cases (printed; numpy's float32 exp may
    differ in the last bit between CPUs, so the restatement is held to half its
    bars, not to the digits)."""
    assert Y.BARS == {k: 4.0 * v for k, v in Y.WORST.items()} and set(Y.BARS) == set(Y.KEYS)
    assert set(S.BARS) - {"image", "v_xy", "v_conic", "v_colors", "v_opacity"} <= set(Y.BARS)
    worst = Y.measure_float32()
    for k, (v, cid) in worst.items():
        print(f"YUV-F32 {k} {v:.3e} {cid} recorded {Y.WORST[k]:.3e}")
    for k, (v, cid) in worst.items():
        assert 0 < v <= 2.0 * Y.WORST[k], (k, v, cid)
