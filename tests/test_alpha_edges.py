"""The alpha compositor's kernels (gsvc_amd/csrc/raster_alpha.hip) on the
scripted cases of tests/alpha_cases.py: partial tiles on both edges, the
per-tile entry counts at which the forward and the backward change code path,
and gradients against references that are not the kernels' own restatement
(float64 autograd of the forward, and a float64 statement of backward.cu's
recursion).  Bars: alpha_cases.BARS (4 x the C oracle's worst error against
float64, tests/analysis/alpha_bars.py).  Every figure is printed before it is
asserted (``ALPHA-ERR`` lines; pytest -s shows them)."""
import numpy as np
import pytest
import torch

import alpha_cases as A

pytestmark = pytest.mark.gpu


def T(a, dev="cuda"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def _tb(c):
    return ((c["W"] + 15) // 16, (c["H"] + 15) // 16, 1)


def _dev(c):
    return [T(c[k]) for k in ("gids", "bins", "xys", "conics", "colors", "opacity", "bg")]


def _forward(c, d):
    from gsvc_amd import ops
    return ops.rasterize_forward(_tb(c), (16, 16, 1), (c["W"], c["H"], 1), *d)


def _backward(c, d, Ts, idx, vo, va):
    from gsvc_amd import ops
    return ops.rasterize_backward(c["H"], c["W"], 16, 16, *d, Ts, idx, T(vo), T(va))


def _report(cid, what, name, value, bar):
    print(f"ALPHA-ERR {cid} {what} {name} {value:.3e} bar {bar:.3e}")


def _check_grads(c, what, got, ref):
    errs = A.grad_errors(c, [N(g) for g in got], ref)
    for name, (whole, edge) in errs.items():
        _report(c["id"], what, name + ".whole", whole, A.BARS[name])
        _report(c["id"], what, name + ".edge", edge, A.BARS[name])
    for name, (whole, edge) in errs.items():
        assert whole <= A.BARS[name] and edge <= A.BARS[name], (what, name, whole, edge)


@pytest.mark.parametrize("cid", A.F64_IDS)
def test_alpha_case_against_float64(cuda, cid):
    """Forward image, T and final_idx against the float64 forward (final_idx
    exact outside the borderline mask, not compared inside it), bit-identical
    over three calls; backward on the kernel's own final_Ts / final_idx, with
    v_out and v_out_alpha zeroed on the borderline pixels, against the
    recursion and -- where no blended alpha nears 0.99 -- autograd, over the
    whole tensors and over the edge splats; its spread over three calls."""
    c = A.BY_ID[cid]
    r = A.reference(cid)
    fwd, keep = r["fwd"], ~r["fwd"]["borderline"]
    d = _dev(c)
    out, Ts, idx = _forward(c, d)
    for _ in range(2):
        o2, t2, i2 = _forward(c, d)
        assert torch.equal(o2, out) and torch.equal(t2, Ts) and torch.equal(i2, idx)
    e_img = float(np.abs(N(out) - fwd["out"])[keep].max())
    e_T = float(np.abs(N(Ts) - fwd["T"])[keep].max())
    _report(cid, "fwd", "image", e_img, A.BARS["image"])
    _report(cid, "fwd", "T", e_T, A.BARS["T"])
    np.testing.assert_array_equal(N(idx)[keep], fwd["idx"][keep])
    assert e_img <= A.BARS["image"] and e_T <= A.BARS["T"]

    runs = [_backward(c, d, Ts, idx, r["v_out"], r["v_alpha"]) for _ in range(3)]
    for name, g0, g1, g2 in zip(A.GRADS, *runs):
        top = float(np.abs(r["rec"][name]).max())
        spread = float(torch.maximum((g1 - g0).abs().max(), (g2 - g0).abs().max())) if g0.numel() else 0.0
        spread = spread / top if top > 0 else spread
        _report(cid, "bwd-spread", name, spread, A.BARS[name])
        assert spread <= A.BARS[name]
    _check_grads(c, "bwd-recursion", runs[0], r["rec"])
    if not fwd["hi99"].any():
        ag = A.alpha_backward64_autograd(c, fwd, r["v_out"], r["v_alpha"])
        _check_grads(c, "bwd-autograd", runs[0], ag)


@pytest.mark.parametrize("cid,kind", A.VARIANT_IDS)
def test_alpha_backward_variants(cuda, cid, kind):
    """v_out alone, v_out_alpha alone, and a caller's final_idx lowered on 10 %
    of the pixels (the kernel's own final_idx, lowered at the same pixels to
    the same positions), against the recursion."""
    c = A.BY_ID[cid]
    fwd = A.reference(cid)["fwd"]
    vo, va, fi, ref = A.variant(cid, kind)
    d = _dev(c)
    _, Ts, idx = _forward(c, d)
    if kind == "lowered":
        low = fi != fwd["idx"]
        idx = torch.where(T(low), T(fi), idx)
    _check_grads(c, "bwd-" + kind, _backward(c, d, Ts, idx, vo, va), ref)


@pytest.mark.parametrize("cid", A.CALLER_IDS)
def test_alpha_caller_geometry_against_oracle(cuda, oracle, cid):
    """A conic that is not positive definite, a needle past cull_conditioned
    and a NaN colour, at op level against the C oracle (float64 is no
    reference there, see alpha_cases), with test_alpha_path's tolerances."""
    c = A.BY_ID[cid]
    d = _dev(c)
    out, Ts, idx = _forward(c, d)
    r_out, r_Ts, r_idx, _ = A.oracle_run(c, c["v_out"], c["v_alpha"])
    np.testing.assert_array_equal(N(idx), r_idx)
    np.testing.assert_allclose(N(out), r_out, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(N(Ts), r_Ts, rtol=1e-5, atol=1e-6)
    assert np.isnan(r_out).any() == (cid == "caller-nancolor")
    got = _backward(c, d, Ts, idx, c["v_out"], c["v_alpha"])
    ref = oracle.raster_backward(_tb(c), c["H"], c["W"], c["gids"], c["bins"], c["xys"], c["conics"],
                                 c["colors"], c["opacity"], c["bg"], N(Ts), N(idx), c["v_out"],
                                 c["v_alpha"])
    for a, b in zip(got, ref):
        b = np.asarray(b, np.float32).reshape(N(a).shape)
        top = float(np.nanmax(np.abs(b)))
        np.testing.assert_allclose(N(a), b, rtol=1e-4, atol=1e-4 * max(1.0, top))


# ---------------------------------------------------------------- the autograd glue
def _glue_inputs(c, **over):
    z = dict(xys=T(c["xys"]), depths=T(c["depths"]), radii=T(c["radii"]), conics=T(c["conics"]),
             nth=T(c["nth"]), colors=T(c["colors"]), opacity=T(c["opacity"]))
    z.update(over)
    for k in ("xys", "conics", "colors", "opacity"):
        if z[k].is_floating_point() and z[k].is_leaf:  # (a view of a leaf carries its own graph)
            z[k].requires_grad_(True)
    return z


def _glue_call(c, z, **kw):
    from gsplat.rasterize import rasterize_gaussians
    return rasterize_gaussians(z["xys"], z["depths"], z["radii"], z["conics"], z["nth"], z["colors"],
                               z["opacity"], c["H"], c["W"], 16, 16, **kw)


def _glue_reference(c, which="both"):
    fwd = A.alpha_forward64(c)
    vo, va = A.upstream(c, fwd["borderline"], which)
    return fwd, vo, va, A.alpha_backward64_recursion(c, fwd["T"], fwd["idx"], vo, va)


def _check_image(cid, what, out, fwd):
    keep = ~fwd["borderline"]
    e = float(np.abs(N(out) - fwd["out"])[keep].max())
    _report(cid, what, "image", e, A.BARS["image"])
    assert e <= A.BARS["image"]


def test_glue_return_alpha_false_and_opacity_shapes(cuda):
    """return_alpha=False (v_out_alpha is None in the backward); opacity of
    shape (N,) and (N, 1): the gradient takes the input's shape."""
    c = A.BY_ID[A.GLUE_ID]
    fwd, vo, va, ref = _glue_reference(c, "out")
    for flat in (False, True):
        z = _glue_inputs(c, opacity=T(c["opacity"].reshape(-1) if flat else c["opacity"]))
        out = _glue_call(c, z, background=T(c["bg"]))
        assert isinstance(out, torch.Tensor) and out.shape == (c["H"], c["W"], 3)
        _check_image(c["id"], "glue-noalpha", out, fwd)
        (out * T(vo)).sum().backward()
        assert z["opacity"].grad.shape == z["opacity"].shape
        _check_grads(c, "glue-noalpha", [z[k].grad for k in ("xys", "conics", "colors", "opacity")], ref)


def test_glue_default_background_is_ones(cuda):
    c = dict(A.BY_ID[A.GLUE_ID], bg=np.ones(3, np.float32))
    fwd, vo, va, ref = _glue_reference(c)
    z = _glue_inputs(c)
    out, alpha = _glue_call(c, z, background=None, return_alpha=True)
    _check_image(c["id"], "glue-bg-none", out, fwd)
    keep = ~fwd["borderline"]
    assert np.abs(N(alpha) - (1.0 - fwd["T"]))[keep].max() <= A.BARS["T"]
    ((out * T(vo)).sum() + (alpha * T(va)).sum()).backward()
    _check_grads(c, "glue-bg-none", [z[k].grad for k in ("xys", "conics", "colors", "opacity")], ref)


def test_glue_uint8_colours_and_strided_inputs(cuda):
    """uint8 colours are colours / 255; non-contiguous xys and colours give
    what their contiguous copies give."""
    base = A.BY_ID[A.GLUE_ID]
    u8 = np.round(base["colors"] * 255).astype(np.uint8)
    c = dict(base, colors=(u8.astype(np.float32) / np.float32(255)))
    fwd, vo, va, ref = _glue_reference(c)
    z = _glue_inputs(c, colors=T(u8))
    out, alpha = _glue_call(c, z, background=T(c["bg"]), return_alpha=True)
    _check_image(c["id"], "glue-uint8", out, fwd)
    ((out * T(vo)).sum() + (alpha * T(va)).sum()).backward()
    # (uint8 colours take no gradient: the reference's own stands in for that slot)
    got = [z["xys"].grad, z["conics"].grad, T(ref["v_colors"]), z["opacity"].grad]
    _check_grads(c, "glue-uint8", got, ref)
    # strided views of wider leaves
    c = base
    fwd, vo, va, ref = _glue_reference(c)
    n = c["xys"].shape[0]
    wide_xy = torch.zeros((n, 4), device="cuda").requires_grad_(True)
    wide_col = torch.zeros((n, 6), device="cuda").requires_grad_(True)
    with torch.no_grad():
        wide_xy[:, ::2] = T(c["xys"])
        wide_col[:, ::2] = T(c["colors"])
    xv, cv = wide_xy[:, ::2], wide_col[:, ::2]
    assert not xv.is_contiguous() and not cv.is_contiguous()
    z = _glue_inputs(c, xys=xv, colors=cv)
    out, alpha = _glue_call(c, z, background=T(c["bg"]), return_alpha=True)
    _check_image(c["id"], "glue-strided", out, fwd)
    ((out * T(vo)).sum() + (alpha * T(va)).sum()).backward()
    assert not wide_xy.grad[:, 1::2].any() and not wide_col.grad[:, 1::2].any()
    got = [wide_xy.grad[:, ::2], z["conics"].grad, wide_col.grad[:, ::2], z["opacity"].grad]
    _check_grads(c, "glue-strided", got, ref)


def test_glue_every_splat_off_screen(cuda):
    """The M < 1 branch: the image is the background and every gradient is
    zero, in the inputs' shapes."""
    c = A.BY_ID[A.GLUE_ID]
    z = _glue_inputs(c, radii=torch.zeros_like(T(c["radii"])), nth=torch.zeros_like(T(c["nth"])))
    out = _glue_call(c, z, background=T(c["bg"]))
    assert torch.equal(out, T(c["bg"]).expand(c["H"], c["W"], 3))
    (out * T(c["v_out"])).sum().backward()
    for k in ("xys", "conics", "colors", "opacity"):
        assert z[k].grad.shape == z[k].shape and not z[k].grad.any()


def test_glue_four_channels_refused(cuda):
    c = A.BY_ID[A.GLUE_ID]
    z = _glue_inputs(c, colors=torch.rand((c["xys"].shape[0], 4), device="cuda"))
    with pytest.raises(NotImplementedError):
        _glue_call(c, z, background=torch.ones(4, device="cuda"))


# ---------------------------------------------------------------- the C ABI
GSVC_OK, GSVC_ERR_ARG = 0, 1


def test_capi_argument_checks(cuda):
    """A block size other than 16 and tile_bounds that do not match the image
    are refused with GSVC_ERR_ARG before anything is launched; a zero-tile
    image returns GSVC_OK."""
    from gsvc_amd import _lib as L
    lib = L.load()
    c = A.BY_ID[A.GLUE_ID]
    H, W = c["H"], c["W"]
    tb = _tb(c)
    d = _dev(c)
    out = torch.full((H, W, 3), 7.0, device="cuda")
    Ts = torch.full((H, W), 7.0, device="cuda")
    idx = torch.full((H, W), 7, dtype=torch.int32, device="cuda")
    rec = torch.full((c["xys"].shape[0], 16), 7.0, device="cuda")
    p = [L.ptr(t) for t in d]
    s = L.stream(cuda)

    def fwd(tbx, tby, bx, by, w, h):
        return lib.gsvc_rasterize_forward(tbx, tby, 1, bx, by, 1, w, h, 1, *p, L.ptr(out), L.ptr(Ts),
                                          L.ptr(idx), s)

    def bwd(h, w, bh, bw):
        return lib.gsvc_rasterize_backward(h, w, bh, bw, c["xys"].shape[0], *p, L.ptr(Ts), L.ptr(idx),
                                           L.ptr(out), L.ptr(Ts), L.ptr(rec), s)

    assert fwd(tb[0], tb[1], 8, 8, W, H) == GSVC_ERR_ARG
    assert fwd(tb[0], tb[1], 16, 8, W, H) == GSVC_ERR_ARG
    assert fwd(tb[0] + 1, tb[1], 16, 16, W, H) == GSVC_ERR_ARG
    assert fwd(tb[0], tb[1] - 1, 16, 16, W, H) == GSVC_ERR_ARG
    assert b"tile" in lib.gsvc_last_error()
    assert bwd(H, W, 8, 16) == GSVC_ERR_ARG
    assert bwd(H, W, 16, 32) == GSVC_ERR_ARG
    torch.cuda.synchronize()
    # nothing was written by a refused call
    assert (out == 7).all() and (Ts == 7).all() and (idx == 7).all() and (rec == 7).all()
    assert fwd(0, 0, 16, 16, 0, 0) == GSVC_OK
    assert fwd(0, tb[1], 16, 16, 0, H) == GSVC_OK
    assert bwd(0, 0, 16, 16) == GSVC_OK
    torch.cuda.synchronize()
    assert (out == 7).all() and not rec.any()  # the backward zeroes the records, launches nothing
