"""GPU: the compression stage's kernels (csrc/quant.hip) against the in-test
restatement of tests/quant_cases.py -- forward and unpack bit for bit, the
fixed-order reductions within the summation bound and identical between runs,
a 3-frame GOP decoded in one launch, the eval render against the oracle, a
short quantized training run, and the stream's argument errors."""
import ctypes

import numpy as np
import pytest
import torch

import quant_cases as Q
from gsvc_amd import compress as C
from gsvc_amd import quantize as QZ

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 257, 4099]  # wave and block edges, and a count that divides nothing
H, W = 40, 72                       # partial tiles on both axes


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def N(t):
    return t.detach().cpu().numpy()


_cases = {}


def case_and_ref(n, delta):
    k = (n, delta)
    if k not in _cases:
        case = Q.make_case(n, delta=delta)
        Q.check_margins(case)  # no colour is ever excused: the margin holds on the reference
        _cases[k] = (case, Q.ref_forward(case))
    return _cases[k]


def run(case, grad=False):
    xyz, chol, feat = (T(case[k]).requires_grad_(grad) for k in ("xyz", "chol", "feat"))
    scale, beta = T(case["scale"]).requires_grad_(grad), T(case["beta"]).requires_grad_(grad)
    prev = None if case["prev"] is None else tuple(T(p) for p in case["prev"])
    out = QZ.quantize_params(xyz, chol, feat, scale, beta, T(case["cb"]), T(case["bound"]), prev)
    return (xyz, chol, feat, scale, beta), out


def model_from_case(case):
    return Q.model_from_case(case, H, W, device="cuda")


@pytest.mark.parametrize("delta", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_forward_bit_equal(cuda, n, delta):
    case, ref = case_and_ref(n, delta)
    _, (xq, Lq, cq, cc, cr, sums) = run(case)
    for got, name in ((xq, "xq"), (Lq, "Lq"), (cq, "cq"), (cc, "codes_chol"), (cr, "codes_rgb")):
        np.testing.assert_array_equal(N(got), ref[name], err_msg=name)
    want = ref["commit_terms"].astype(np.float64).sum(0)
    err = np.abs(N(sums).astype(np.float64) - want)
    print("commit sums", n, err, Q.sum_bound(ref["commit_terms"]))
    assert (err <= Q.sum_bound(ref["commit_terms"])).all()
    _, again = run(case)
    np.testing.assert_array_equal(N(again[5]), N(sums))  # identical bits across two runs
    # without the sums (inference, encoding) the other kernel variant gives the same bits
    prev = None if case["prev"] is None else tuple(T(p) for p in case["prev"])
    lean = QZ.quantize_params(*(T(case[k]) for k in ("xyz", "chol", "feat", "scale", "beta", "cb",
                                                       "bound")), prev, commit=False)
    assert lean[5] is None
    for a, b in zip(lean[:5], (xq, Lq, cq, cc, cr)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("n", SIZES)
def test_backward(cuda, n):
    """Longest addition path of the reductions as built: quant_cases.longest_path
    (1 + 6 + 3 + blocks - 1 for these sizes: 10 .. 26 additions), smaller than
    N - 1 from N = 12 on, so the tighter bound applies there."""
    case, ref = case_and_ref(n, False)
    v_xq, v_Lq, v_cq, v_commit = Q.upstream(n)
    grads = []
    for vc in (np.zeros(2, np.float32), v_commit, v_commit):
        (xyz, chol, feat, scale, beta), (xq, Lq, cq, _, _, sums) = run(case, grad=True)
        ((xq * T(v_xq)).sum() + (Lq * T(v_Lq)).sum() + (cq * T(v_cq)).sum()
         + (sums * T(vc)).sum()).backward()
        grads.append([N(g.grad) for g in (xyz, chol, feat, scale, beta)])
    want = Q.ref_backward(case, ref, v_xq, v_Lq, v_cq, v_commit)
    st, full, again = grads
    np.testing.assert_array_equal(st[0], want["v_xyz"])
    np.testing.assert_array_equal(st[1], want["v_chol"])
    np.testing.assert_array_equal(st[2], want["v_feat_st"])  # the straight-through part: 2 v_cq
    np.testing.assert_array_equal(full[2], want["v_feat"])   # with the commitment term, same op order
    for got, terms, name in ((full[3], want["t_scale"], "v_scale"), (full[4], want["t_beta"], "v_beta")):
        ref64 = terms.astype(np.float64).sum(0)
        err, bound = np.abs(got.astype(np.float64) - ref64), Q.sum_bound(terms)
        print(name, n, "err", err, "bound", bound)
        assert (err <= bound).all(), (name, err, bound)
    for a, b in zip(full, again):  # identical bits across two runs
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(st[3], full[3])


@pytest.mark.parametrize("n", SIZES)
def test_unpack_of_pack_bit_equal_forward(cuda, n):
    """unpack(pack(model)) gives the forward kernel's xq, Lq, cq: a key frame,
    and a delta frame on the key frame's decoded parameters (a frame stream of
    odd length puts the second frame at an odd byte offset)."""
    key, ref0 = case_and_ref(n, False)
    mk = model_from_case(key)
    s0 = C.encode_frame(mk)
    assert len(s0) == C.HEADER_BYTES + 7 * n
    # the pack kernel wrote what the host packer restates
    assert s0[C.HEADER_BYTES:] == Q.ref_planes(key["xyz"], ref0["codes_chol"], ref0["codes_rgb"])
    with torch.no_grad():
        fwd0 = mk.quantized()
    xq, Lq, cq, Lpre, sizes, hw = C.unpack_frames([s0], "cuda")
    assert sizes == [n] and hw == (H, W)
    for got, f, name in ((xq, fwd0[0], "xq"), (Lq, fwd0[1], "Lq"), (cq, fwd0[2], "cq")):
        assert torch.equal(got, f), name
        np.testing.assert_array_equal(N(got), ref0[name])
    np.testing.assert_array_equal(N(Lpre), ref0["Lpre"])
    delta = dict(Q.make_case(n, seed=1, delta=True))
    delta["prev"] = (ref0["xq"], ref0["Lpre"], ref0["cq"])
    md = model_from_case(delta)
    s1 = C.encode_frame(md)
    with torch.no_grad():
        fwd1 = md.quantized()
    xq, Lq, cq, Lpre, sizes, _ = C.unpack_frames([s0, s1], "cuda")
    assert sizes == [n, n]
    for got, f, name in ((xq, fwd1[0], "xq"), (Lq, fwd1[1], "Lq"), (cq, fwd1[2], "cq")):
        assert torch.equal(got[n:], f), name
        assert torch.equal(got[:n], fwd0[("xq", "Lq", "cq").index(name)]), name
    # the second frame alone, on the state carried from the first call
    state = (T(ref0["xq"]), T(ref0["Lpre"]), T(ref0["cq"]))
    xq2, Lq2, cq2, _, _, _ = C.unpack_frames([s1], "cuda", prev=state)
    assert torch.equal(xq2, fwd1[0]) and torch.equal(Lq2, fwd1[1]) and torch.equal(cq2, fwd1[2])


def _gop():
    """One key frame and two delta frames of different sizes; each delta model
    holds the decoded parameters of the frame before it (its first N splats)."""
    torch.manual_seed(5)
    kw = dict(H=H, W=W, BLOCK_H=16, BLOCK_W=16, device="cuda", lr=1e-3, quantize=True, opt_type="adan")
    models, streams, state = [], [], None
    for n in (257, 200, 65):
        if state is None:
            m = C.GaussianVideoFrameQ(num_points=n, **kw).cuda()
            with torch.no_grad():
                m._cholesky.mul_(3.0)
        else:
            m = C.GaussianVideoDelta(num_points=n, **kw).cuda()
            with torch.no_grad():
                m._xyz.copy_(0.05 * torch.randn(n, 2))
                m._cholesky.copy_(0.3 * torch.randn(n, 3))
                m._features_dc.copy_(0.1 * torch.randn(n, 3))
                m.p_xyz.copy_(state[0][:n])
                m.p_cholesky.copy_(state[1][:n])
                m.p_features_dc.copy_(state[2][:n])
        m._init_data()
        m.eval()
        s = C.encode_frame(m)
        xq, _, cq, Lpre, _, _ = C.unpack_frames([s], "cuda", prev=state)
        state = (xq, Lpre, cq)
        models.append(m)
        streams.append(s)
    return models, streams


def test_gop_decode_bit_equal(cuda):
    from gsvc_amd.render import render_frame_sum
    models, streams = _gop()
    imgs = C.decode_frames(streams, "cuda")
    assert imgs.shape == (3, 3, H, W)
    xq, Lq, cq, _, sizes, _ = C.unpack_frames(streams, "cuda")
    assert sizes == [257, 200, 65]
    o = 0
    bg = torch.ones(3, device="cuda")
    for f, m in enumerate(models):
        with torch.no_grad():
            out = m.forward_quantize()
        assert torch.equal(imgs[f], out["render"][0]), f
        one = render_frame_sum(xq[o:o + sizes[f]], Lq[o:o + sizes[f]], cq[o:o + sizes[f]], H, W, bg,
                               xyz_tanh=True, cholesky_bound=None)
        assert torch.equal(imgs[f], one[0]), f
        # training mode's op path (tanh in torch, project, rasterize) renders the same bits
        with torch.enable_grad():
            ops = m._render(torch.tanh(xq[o:o + sizes[f]]), Lq[o:o + sizes[f]], cq[o:o + sizes[f]])
        assert torch.equal(ops.detach()[0], imgs[f]), f
        o += sizes[f]
    assert float(imgs.min()) >= 0 and float(imgs.max()) <= 1 and float(imgs.std()) > 0


def _render_case(delta):
    """The hard-case inputs with splats small enough that most pixels stay
    inside the clamp and none is near-degenerate (where the image magnifies an
    ulp of tanh past the tolerance): a quarter of the quantizer's scale and
    another dyadic beta (the raw codes stay exact), smaller previous-frame
    parameters."""
    case = dict(Q.make_case(257, seed=2, delta=delta))
    raw = (case["chol"] - case["beta"][None]) / case["scale"][None]
    case["scale"] = case["scale"] / np.float32(4)
    case["beta"] = np.array([0.25, -0.25, 0.25], np.float32)  # no near-degenerate splat
    case["chol"] = case["beta"][None] + raw * case["scale"][None]
    if delta:
        p = case["prev"]
        case["prev"] = (p[0], p[1] * np.float32(0.25), p[2] * np.float32(0.3))
    Q.check_margins(case)
    return case


@pytest.mark.parametrize("delta", [False, True])
def test_eval_render_matches_oracle(cuda, oracle, delta):
    """The eval render against oracle.render_sum of the restated dequantized
    parameters, at the project's image tolerance."""
    n = 257
    case = _render_case(delta)
    ref = Q.ref_forward(case)
    m = model_from_case(case)
    with torch.no_grad():
        img = m.forward_quantize()["render"]
    want = oracle.render_sum(np.tanh(ref["xq"]).astype(np.float32), ref["Lq"], ref["cq"],
                             np.ones((n, 1), np.float32), H, W)["out"]
    assert ((want > 0) & (want < 1)).mean() > 0.5  # the clamp does not hide the image
    want = np.clip(want, 0, 1).transpose(2, 0, 1)[None]
    np.testing.assert_allclose(N(img), want, rtol=1e-6, atol=1e-5)


def _train(seed, steps):
    from gsvc_amd.frame import synthetic_gt
    torch.manual_seed(seed)
    gt = synthetic_gt(H, W, 3, "cuda")
    m = C.GaussianVideoFrameQ(num_points=257, H=H, W=W, BLOCK_H=16, BLOCK_W=16, device="cuda",
                              lr=1e-2, quantize=True, opt_type="adan").cuda()
    with torch.no_grad():
        m._cholesky.mul_(4.0)
    m._init_data()
    m.train()
    hist = []
    for _ in range(steps):
        loss, psnr = m.train_iter_quantize(gt)
        hist.append((loss.item(), psnr))
    return hist


def test_quantized_training_steps(cuda):
    a = _train(11, 20)
    b = _train(11, 1)
    assert all(np.isfinite(l) and np.isfinite(p) for l, p in a)
    assert a[0] == b[0]  # equal seeds: the first step's loss and PSNR, bit for bit
    print("psnr", a[0][1], "->", a[-1][1])
    assert a[-1][1] >= a[0][1]


def test_compress_video_round_trip(cuda):
    """compress_video on three tiny frames (a key frame and two deltas, the
    second with fewer splats): with deltas trained against the decoder's state
    the decoded GOP reproduces the PSNR the loop measured, exactly; with the
    reference's overfit targets the streams still decode, to other images."""
    import math
    from gsvc_amd.frame import synthetic_gt
    torch.manual_seed(3)
    frames = [synthetic_gt(H, W, s, "cuda") for s in (1, 2, 3)]
    sd = {}
    for i, n in enumerate((65, 65, 40)):
        sd[f"frame_{i + 1}"] = {"_xyz": torch.atanh(2 * (torch.rand(n, 2) - 0.5)).cuda(),
                                "_cholesky": (3 * torch.rand(n, 3)).cuda(),
                                "_features_dc": torch.rand(n, 3).cuda()}
    out = C.compress_video(sd, frames, K_frames=[1], iterations=3, lr=1e-2, device="cuda",
                           delta_base="decoded", seed=0)
    assert [len(s) for s in out["streams"]] == [256 + 7 * 65, 256 + 7 * 65, 256 + 7 * 40]
    assert [C.parse_header(s)["delta"] for s in out["streams"]] == [False, True, True]
    imgs = C.decode_frames(out["streams"], "cuda")
    for f in range(3):
        mse = torch.nn.functional.mse_loss(imgs[f:f + 1], frames[f]).item()
        assert 10 * math.log10(1.0 / mse) == out["psnr"][f], f
        assert out["bpp"][f] == 8 * len(out["streams"][f]) / H / W
        assert 0 < out["bpp_entropy_estimate"][f]
    ref = C.compress_video(sd, frames, K_frames=[1], iterations=3, lr=1e-2, device="cuda",
                           delta_base="overfit", seed=0)
    # Two training runs are not bit-identical past their first step (the render
    # backward's gradients meet through float atomics), so the trained tables
    # and codes of the two runs may differ: only what training does not touch
    # is compared.
    for a, b in zip(ref["streams"], out["streams"]):
        ha, hb = C.parse_header(a), C.parse_header(b)
        assert [ha[k] for k in ("N", "H", "W", "delta")] == [hb[k] for k in ("N", "H", "W", "delta")]
    drift = C.decode_frames(ref["streams"], "cuda")
    assert drift.shape == imgs.shape and bool(torch.isfinite(drift).all())
    assert set(ref["state_dicts"]["frame_2"]) == {"_xyz", "_cholesky", "_features_dc"}


def test_nan_cholesky_gives_code_zero(cuda):
    """fmaxf(raw, 0) drops a NaN: code 0 and Lq = beta + bound, on both dispatches."""
    case = dict(Q.make_case(5))
    case["chol"] = case["chol"].copy()
    case["chol"][2, 1] = np.nan
    _, (xq, Lq, cq, cc, cr, _) = run(case)
    assert int(cc[2, 1]) == 0
    assert float(Lq[2, 1]) == float(case["beta"][1] + case["bound"][1])
    np.testing.assert_array_equal(N(Lq)[[0, 1, 3, 4]], Q.ref_forward(Q.make_case(5))["Lq"][[0, 1, 3, 4]])


def test_argument_errors_launch_nothing(cuda):
    from gsvc_amd import _lib
    lib = _lib.load()
    good = C.encode_frame(model_from_case(case_and_ref(65, False)[0]))
    out = torch.full((65 * 8,), 7.0, device="cuda")
    bound = torch.tensor([0.5, 0.0, 0.5], device="cuda")

    def call(buf, prev_n=0):
        buf = bytes(buf)
        arr = (ctypes.c_longlong * 2)(0, len(buf))
        dev = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
        p = ctypes.c_void_p(out.data_ptr())
        rc = lib.gsvc_unpack_splats(1, ctypes.c_char_p(buf), arr, ctypes.c_void_p(dev.data_ptr()),
                                    ctypes.c_void_p(bound.data_ptr()), None, None, None, prev_n,
                                    p, p, p, None, 65, None)
        torch.cuda.synchronize()
        return rc

    bad = bytearray(good)
    bad[1] ^= 0x10
    neg = bytearray(good)
    neg[8:12] = (-1).to_bytes(4, "little", signed=True)
    dl = bytearray(good)
    dl[20] = 1
    for buf, msg in ((bad, b"magic"), (good[:-7], b"truncated"), (good[:17], b"truncated"),
                     (neg, b"N < 0"), (dl, b"no predecessor")):
        assert call(buf) == 1 and msg in lib.gsvc_last_error(), msg
    assert call(dl, prev_n=3) == 1 and b"previous-frame" in lib.gsvc_last_error()
    assert bool((out == 7.0).all())  # nothing was launched
    with pytest.raises(ValueError, match="magic"):
        C.decode_frames([bytes(bad)], "cuda")
    z = torch.zeros(0, 2, device="cuda")
    z3 = torch.zeros(0, 3, device="cuda")
    one = torch.ones(3, device="cuda")
    cb = torch.zeros(2, 8, 3, device="cuda")
    xq, Lq, cq, cc, cr, sums = QZ.quantize_params(z, z3, z3, one, one, cb, one)
    assert xq.shape == (0, 2) and cr.shape == (0, 2) and float(sums.abs().sum()) == 0
