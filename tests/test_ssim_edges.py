"""SSIM / MS-SSIM kernels (csrc/ssim.hip behind gsvc_amd/msssim.py) at tile
edges, every window size, short dimensions, clamped planes and non-default
options -- the cases of tests/ssim_cases.py.

References.  Values: the float64 numpy oracle (oracle.ssim / oracle.ms_ssim).
Gradients w.r.t. X and Y: CPU float64 autograd through the torch restatement of
test_ssim.py (float64 window), upstream linspace(0.5, 1.5, B) on the per-image
output.  A plane with a clamped term (relu at a level of MS-SSIM, or
nonnegative_ssim) has value 0 and, by the kernels' convention relu'(0) = 0,
gradient exactly 0; torch's own autograd gives NaN there (0 ** (w - 1) times
relu'), so the reference leaves those planes out of its sum.  Which planes clamp
is asserted on the float64 reference first (ssim_cases.CLAMPED), together with
every raw term of those inputs lying outside (-0.5, 0.3), away from the kink
(the 5-level case on that input: outside (-0.3, 0.3), ssim_cases.KINK).

Bars.  Per family, 4 times the worst error of the *fp32 restatement* on the CPU
against the float64 reference over the family's cases (tests/analysis/
ssim_bars.py prints them); the factor covers the kernels' different summation
order and fma contraction.  Values: absolute.  Gradients: the largest error
over the tensor relative to the reference's largest element, and the largest
error over the outer band of width win_size - 1 relative to the band's largest
reference element -- the same bar for both (the border is where few windows
overlap, gradients are small and the transposed filter's index arithmetic can go
wrong).

    family               fp32 restatement, worst       kernels on an MI355X, worst
                         value    grad     band        value    grad     band
    SSIM                 2.5e-07  4.7e-06  8.6e-06     2.5e-07  4.2e-06  7.0e-06
    MS-SSIM              8.9e-07  2.7e-05  2.6e-05     1.4e-06  3.2e-05  2.5e-05
    data_range 255       7.8e-07  2.1e-05  7.5e-06     1.8e-07  2.3e-05  7.7e-06

(SSIM's worst gradient figures are the unfiltered cases -- win_size 1, and 5x9
under window 11 -- where cs is identically 1 and its three O(1 / C2) gradient
terms cancel; filtered cases stay below 3e-06.)  The bar of each gradient
family is 4 times its "grad" column; the numbers are RESTATEMENT_WORST and BAR
of test_ssim.py, which holds its own cases to them too.
"""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import ssim_cases as S
from test_ssim import BAR, _pair

_refs = {}


def ref_of(cid, avg=False, want=(True, True)):
    """The float64 reference of a case, computed once and shared."""
    key = (cid, avg, want)
    if key not in _refs:
        _refs[key] = S.reference(S.BY_ID[cid], avg=avg, want=want)
    return _refs[key]


def call(c, X, Y, avg=False):
    """The kernels on (X, Y) with the case's options; the "Skipping Gaussian
    Smoothing" warning is raised exactly as often as the case says."""
    from gsvc_amd.msssim import ms_ssim, ssim
    fn = ssim if c["kind"] == "ssim" else ms_ssim
    if c["warns"]:
        with pytest.warns(UserWarning, match="Skipping Gaussian Smoothing") as rec:
            out = fn(X, Y, size_average=avg, **c["opts"])
        assert len(rec) == c["warns"]
        return out
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        return fn(X, Y, size_average=avg, **c["opts"])


def run(c, cuda, avg=False, want=(True, True)):
    """(value, dX, dY) of the kernels for the reference's upstream."""
    X, Y = S.inputs(c)
    X = X.to(cuda).requires_grad_(want[0])
    Y = Y.to(cuda).requires_grad_(want[1])
    out = call(c, X, Y, avg)
    loss = out if avg else (out * S.upstream(out.numel(), torch.float32).to(cuda)).sum()
    loss.backward()
    return out.detach(), X.grad, Y.grad


def check(c, ref, got, oracle_value):
    """Value against the oracle, gradients against the reference: whole tensor
    and outer band on the planes that do not clamp, exactly 0 on those that do."""
    val, dX, dY = got
    bar_v, bar_g = BAR[c["family"]]
    win = c["opts"].get("win_size", 11)
    assert sorted(map(tuple, ref["clamped"].nonzero().tolist())) == S.CLAMPED.get(c["id"], [])
    if ref["clamped"].any() or c["id"] in S.KINK:
        lo, hi = S.KINK[c["id"]]
        assert bool(((ref["raw"] <= lo) | (ref["raw"] >= hi)).all()), ref["raw"]
    ev = float(np.abs(val.cpu().double().numpy() - oracle_value).max())
    figs = [ev]
    keep = ~ref["clamped"]
    for name, g, r in (("dX", dX, ref["dX"]), ("dY", dY, ref["dY"])):
        if r is None:
            assert g is None
            figs += [float("nan")] * 2
            continue
        assert bool(torch.isfinite(g).all()), name
        if ref["clamped"].any():
            assert float(g.cpu()[ref["clamped"]].abs().max()) == 0.0, name
        figs += S.grad_errors(g, r, win, keep)
    print("FIG %-12s %-8s value %.2e  dX %.2e band %.2e  dY %.2e band %.2e"
          % ((c["id"], c["family"]) + tuple(figs)))
    assert ev <= bar_v, (ev, bar_v)
    assert all(e <= bar_g for e in figs[1:] if e == e), (figs, bar_g)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c["id"] for c in S.CASES])
def test_value_and_gradients(cuda, oracle, cid):
    """Per-image output and its gradients w.r.t. X and Y, every case."""
    c = S.BY_ID[cid]
    check(c, ref_of(cid), run(c, cuda), S.oracle_value(oracle, c))


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["t-27x75", "p270", "anti-nonneg", "m-w3", "m-anti3", "m-anti"])
def test_size_average(cuda, oracle, cid):
    """size_average=True: the mean over all planes, upstream 1."""
    c = S.BY_ID[cid]
    got = run(c, cuda, avg=True)
    assert got[0].shape == ()
    check(c, ref_of(cid, avg=True), got, S.oracle_value(oracle, c, avg=True))


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["t-27x75", "m-w3"])
def test_gradient_to_y_alone(cuda, oracle, cid):
    """X does not require a gradient: dY is computed on its own."""
    c = S.BY_ID[cid]
    got = run(c, cuda, want=(False, True))
    assert got[1] is None
    check(c, ref_of(cid, want=(False, True)), got, S.oracle_value(oracle, c))


@pytest.mark.gpu
def test_single_weight_is_multi_scale(cuda, oracle):
    """ms_ssim(weights=[w]) is relu(ssim) ** w per plane, not the plain mean
    SSIM: the two are 100 bars apart on this input, so the case can tell.  (With
    the branch chosen by the level count the kernels returned the plain SSIM,
    0.9400 / 0.9383 against 0.9576 / 0.9564.)"""
    from gsvc_amd.msssim import ms_ssim
    c = S.BY_ID["m-L1"]
    X, Y = S.inputs(c)
    per_plane = ref_of("m-L1")["raw"][0]
    want = (torch.relu(per_plane) ** 0.7).mean(1).numpy()
    plain = oracle.ssim(X.numpy(), Y.numpy(), 1.0, size_average=False, win_size=3)
    np.testing.assert_allclose(S.oracle_value(oracle, c), want, rtol=0, atol=1e-12)
    assert np.abs(want - plain).min() > 100 * BAR["ms"][0]
    got = ms_ssim(X.to(cuda), Y.to(cuda), data_range=1, size_average=False, win_size=3,
                  weights=[0.7])
    np.testing.assert_allclose(got.cpu().double().numpy(), want, rtol=0, atol=BAR["ms"][0])


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["m-L1", "m-L3", "m-L8"])
def test_weights_as_tensor(cuda, cid):
    """`weights` as a tensor gives the bits of the same weights as a list."""
    c = S.BY_ID[cid]
    tc = dict(c, opts=dict(c["opts"], weights=torch.tensor(c["opts"]["weights"], dtype=torch.float64)))
    a, b = run(c, cuda), run(tc, cuda)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.gpu
def test_modules_equal_functions(cuda):
    from gsvc_amd.msssim import MS_SSIM, SSIM, ms_ssim, ssim
    X, Y = _pair((2, 3, 65, 49), 12)
    X, Y = (255 * X).to(cuda), (255 * Y).to(cuda)
    kw = dict(data_range=255, size_average=False, win_size=7, win_sigma=1.2, K=(0.02, 0.04))
    a = SSIM(channel=3, nonnegative_ssim=True, **kw)(X, Y)
    assert a.shape == (2,) and torch.equal(a, ssim(X, Y, nonnegative_ssim=True, **kw))
    kw.update(win_size=3, weights=[0.3, 0.3, 0.4])
    a = MS_SSIM(channel=3, **kw)(X, Y)
    assert a.shape == (2,) and torch.equal(a, ms_ssim(X, Y, **kw))
    # and the non-default arguments are not ignored
    assert not torch.equal(a, ms_ssim(X, Y, **dict(kw, K=(0.01, 0.03))))
    assert not torch.equal(a, ms_ssim(X, Y, **dict(kw, win_sigma=1.5)))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float64])
def test_other_dtypes_run_in_fp32(cuda, dtype):
    """The output (and the gradients) carry the input's dtype; the value is the
    fp32 kernels' on X.float(), cast back."""
    from gsvc_amd.msssim import ms_ssim, ssim
    X, Y = _pair((2, 3, 65, 49), 13)
    X, Y = X.to(cuda).to(dtype), Y.to(cuda).to(dtype)
    for fn, kw in ((ssim, dict(win_size=11)), (ms_ssim, dict(win_size=3))):
        xa, ya = X.clone().requires_grad_(True), Y.clone().requires_grad_(True)
        xf, yf = X.float().requires_grad_(True), Y.float().requires_grad_(True)
        a = fn(xa, ya, data_range=1, size_average=False, **kw)
        f = fn(xf, yf, data_range=1, size_average=False, **kw)
        assert a.dtype == dtype and f.dtype == torch.float32
        assert torch.equal(a, f.to(dtype))
        a.sum().backward()
        f.sum().backward()
        assert xa.grad.dtype == dtype and ya.grad.dtype == dtype
        assert torch.equal(xa.grad, xf.grad.to(dtype)) and torch.equal(ya.grad, yf.grad.to(dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("multi", [False, True])
def test_permuted_view_equals_contiguous_copy(cuda, multi):
    """The render is an [H, W, C] image seen as [1, C, H, W]: same bits as its
    contiguous copy, forward and gradient."""
    from gsvc_amd.msssim import ms_ssim, ssim
    X, Y = _pair((1, 3, 65, 49), 14)
    img = X[0].permute(1, 2, 0).contiguous().to(cuda).requires_grad_(True)   # [H, W, C]
    gt = Y[0].permute(1, 2, 0).contiguous().to(cuda).requires_grad_(True)
    xv, yv = img.permute(2, 0, 1).unsqueeze(0), gt.permute(2, 0, 1).unsqueeze(0)
    assert not xv.is_contiguous()
    xc = xv.detach().contiguous().requires_grad_(True)
    yc = yv.detach().contiguous().requires_grad_(True)
    fn = (lambda a, b: ms_ssim(a, b, data_range=1, win_size=3)) if multi else \
        (lambda a, b: ssim(a, b, data_range=1))
    v, c = fn(xv, yv), fn(xc, yc)
    assert torch.equal(v, c)
    v.backward()
    c.backward()
    assert torch.equal(img.grad.permute(2, 0, 1).unsqueeze(0), xc.grad)
    assert torch.equal(gt.grad.permute(2, 0, 1).unsqueeze(0), yc.grad)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["t-27x75", "p270", "m-162x200", "m-L1", "m-anti"])
def test_run_to_run_bit_identical(cuda, cid):
    """The reductions have a fixed order: two calls give the same bits."""
    c = S.BY_ID[cid]
    a, b = run(c, cuda), run(c, cuda)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.gpu
def test_identical_images(cuda):
    """ssim(X, X) is exactly 1 (cs and l are quotients of equal floats), and its
    gradient is 0 within the SSIM bar of the largest gradient element of the
    noisy pair at the same shape (the fp32 restatement: 8.6e-7 of it)."""
    from gsvc_amd.msssim import ssim
    c = S.BY_ID["t-27x75"]
    scale = float(ref_of("t-27x75")["dX"].abs().max())
    X = S.inputs(c)[0].to(cuda).requires_grad_(True)
    out = ssim(X, X, data_range=1, size_average=False)
    assert out.tolist() == [1.0, 1.0]
    (out * S.upstream(2, torch.float32).to(cuda)).sum().backward()
    e = float(X.grad.abs().max()) / scale
    print("FIG X-is-Y grad / scale %.2e" % e)
    assert e <= BAR["ssim"][1]


# ---------------------------------------------------------------- C ABI

def _abi(cuda):
    """The library, a 1 x 2 x 20 x 30 pair on the device and a sentinel-filled `out`."""
    from gsvc_amd import _lib
    X, Y = _pair((1, 2, 20, 30), 15)
    out = torch.full((1,), -7.0, device=cuda)
    torch.cuda.synchronize()
    return _lib.load(), X.to(cuda), Y.to(cuda), out


@pytest.mark.gpu
def test_capi_short_workspace_launches_nothing(cuda):
    """gsvc_ssim_forward with a workspace one byte short returns the workspace
    error and leaves `out` as it was; with the full size it runs."""
    lib, X, Y, out = _abi(cuda)
    need = lib.gsvc_ssim_workspace_bytes(2, 20, 30, 11, 1)
    assert need > 0
    ws = torch.empty((need,), dtype=torch.uint8, device=cuda)
    args = [1, 2, 20, 30, X.data_ptr(), Y.data_ptr(), 11, 1.5, 1e-4, 9e-4, 1, None, 0,
            out.data_ptr(), ws.data_ptr()]
    assert lib.gsvc_ssim_forward(*args, need - 1, None) == 2
    assert b"workspace" in lib.gsvc_last_error()
    torch.cuda.synchronize()
    assert out.tolist() == [-7.0]
    assert lib.gsvc_ssim_forward(*args, need, None) == 0
    torch.cuda.synchronize()
    assert 0.5 < out.item() < 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("levels", [0, 9])
def test_capi_levels_out_of_range(cuda, levels):
    """levels outside 1..8: an argument error before any launch, and the size
    queries answer 0."""
    lib, X, Y, out = _abi(cuda)
    ws = torch.empty((1 << 16,), dtype=torch.uint8, device=cuda)
    w = (ctypes.c_double * 9)(*([0.1] * 9))
    rc = lib.gsvc_ssim_forward(1, 2, 20, 30, X.data_ptr(), Y.data_ptr(), 3, 1.5, 1e-4, 9e-4,
                               levels, w, 0, out.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert rc == 1 and b"levels" in lib.gsvc_last_error()
    torch.cuda.synchronize()
    assert out.tolist() == [-7.0]
    assert lib.gsvc_ssim_workspace_bytes(2, 20, 30, 3, levels) == 0
    assert lib.gsvc_ssim_backward_scratch_bytes(2, 20, 30, 3, levels) == 0
