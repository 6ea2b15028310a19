"""Cases and helpers of the resampled render's tests (test_resample_cpu.py,
test_resample_gpu.py): small frame models, each there for a reason, the views
whose results are known exactly from the native render, and the numpy
restatement of the sampling rule (include/gsvc_amd.h
gsvc_render_frames_resampled)."""
import numpy as np
import torch

BOUND = (0.5, 0.0, 0.5)
# the image bar of the GPU-forward-against-CPU / oracle tests
# (tests/test_gpu_parity.py, tests/test_cpu_path.py: out_img)
IMG_RTOL, IMG_ATOL = 1e-6, 1e-5


def _params(n, gen, chol_scale=1.0):
    means = torch.tanh(1.2 * torch.randn(n, 2, generator=gen))
    chol = (torch.rand(n, 3, generator=gen) * torch.tensor([2.0, 1.0, 2.0]) +
            torch.tensor([0.3, -0.5, 0.3])) * chol_scale
    col = torch.rand(n, 3, generator=gen) * 0.5
    return means, chol, col


def _case(name):
    """{H, W, sizes, means [N,2] (activated), chol [N,3] (without the bound),
    col [N,3], bg [3]} on the CPU."""
    gen = torch.Generator().manual_seed({"edge": 11, "piled": 12, "batch": 13, "wide": 14}[name])
    bg = torch.ones(3)
    if name == "edge":  # partial edge tiles, W % 4 != 0
        H, W, sizes = 37, 53, [150]
        means, chol, col = _params(150, gen)
    elif name == "piled":  # tiles past 256 and past 1024 entries: the native cut
        H, W, n = 64, 64, 6000
        sizes = [n]
        means, chol, col = _params(n, gen)
        sel = torch.arange(0, n, 4)
        means[sel] = -0.25 + 0.05 * torch.rand(len(sel), 2, generator=gen)
        chol[sel] = torch.tensor([2.5, 0.3, 1.5]) - torch.tensor(BOUND)
    elif name == "batch":  # three frames of different N, the middle one all-degenerate (M = 0)
        H, W, sizes = 72, 120, [400, 90, 250]
        means, chol, col = _params(sum(sizes), gen)
        chol[400:490] = -torch.tensor(BOUND)  # L = 0: no splat visible
        bg = torch.tensor([0.25, 1.5, -0.5])
    elif name == "wide":  # wide splats over many tiles
        H, W, sizes = 256, 256, [3000]
        means, chol, col = _params(3000, gen, chol_scale=8.0)
    else:
        raise KeyError(name)
    return dict(name=name, H=H, W=W, sizes=sizes, means=means.contiguous(), chol=chol.contiguous(),
                col=col.contiguous(), bg=bg)


_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = _case(name)
    return _cases[name]


CASES = ("edge", "piled", "batch", "wide")
# integer windows (x0, y0, w, h) at scale 1
CROPS = {"edge": (5, 19, 31, 17), "piled": (16, 0, 40, 64), "batch": (33, 7, 50, 41),
         "wide": (70, 90, 96, 80)}
# (case, k, cropped): odd upscales whose samples k j + (k - 1) / 2 are the native ones
UPSCALES = [(c, k, cr) for c in ("edge", "piled", "batch") for k in (3, 5) for cr in (False, True)]
UPSCALES += [("wide", 3, False), ("wide", 3, True), ("wide", 5, True)]
UPSCALES_CPU = [u for u in UPSCALES if u[0] != "wide"] + [("wide", 3, True)]


def render(c, device, view=None):
    """render_frames_sum of the case on ``device`` (activated means)."""
    from gsvc_amd.render import render_frames_sum
    t = lambda x: x.to(device)
    return render_frames_sum(t(c["means"]), t(c["chol"]), t(c["col"]), c["sizes"], c["H"], c["W"],
                             t(c["bg"]), xyz_tanh=False, cholesky_bound=t(torch.tensor(BOUND)), view=view)


def native_cpu(c):
    """The case's native render on the CPU, frame by frame through the CPU
    operators (as decode_frames on a CPU device): [F, 3, H, W] clamped."""
    from gsvc_amd.project_gaussians_2d import project_gaussians_2d
    from gsvc_amd.rasterize_sum import rasterize_gaussians_sum
    H, W = c["H"], c["W"]
    tb = ((W + 15) // 16, (H + 15) // 16, 1)
    imgs, a = [], 0
    for n in c["sizes"]:
        sl = slice(a, a + n)
        a += n
        xys, depths, radii, conics, nth = project_gaussians_2d(
            c["means"][sl], c["chol"][sl] + torch.tensor(BOUND), H, W, tb)
        img = rasterize_gaussians_sum(xys, depths, radii, conics, nth, c["col"][sl], torch.ones(n, 1),
                                      H, W, 16, 16, background=c["bg"], return_alpha=False)
        imgs.append(torch.clamp(img, 0, 1).view(H, W, 3).permute(2, 0, 1))
    return torch.stack(imgs).contiguous()


def window(native, crop):
    x0, y0, w, h = crop
    return native[..., y0:y0 + h, x0:x0 + w]


# --------------------------------------------------------------------------
# a 3-frame stream with two delta frames

STREAM_H, STREAM_W = 48, 80
STREAM_PLAN = ((300, True), (300, False), (260, False))
_stream = []


def stream():
    """Frame streams of untrained models built on the CPU (as
    test_yuv_out_cpu's _gop_cpu): every delta model holds the decoded
    parameters of the frame before it; versions 1 and 2 alternate."""
    if _stream:
        return _stream[0]
    from gsvc_amd import compress as C
    torch.manual_seed(21)
    kw = dict(H=STREAM_H, W=STREAM_W, BLOCK_H=16, BLOCK_W=16, device="cpu", lr=1e-3, quantize=True,
              opt_type="adan")
    streams, state = [], None
    for k, (n, key) in enumerate(STREAM_PLAN):
        if key:
            m = C.GaussianVideoFrameQ(num_points=n, **kw)
            with torch.no_grad():
                m._cholesky.mul_(3.0)
            state = None
        else:
            m = C.GaussianVideoDelta(num_points=n, **kw)
            with torch.no_grad():
                m._xyz.copy_(0.05 * torch.randn(n, 2))
                m._cholesky.copy_(0.3 * torch.randn(n, 3))
                m._features_dc.copy_(0.1 * torch.randn(n, 3))
                m.p_xyz.copy_(torch.from_numpy(state[0][:n]))
                m.p_cholesky.copy_(torch.from_numpy(state[1][:n]))
                m.p_features_dc.copy_(torch.from_numpy(state[2][:n]))
        m._init_data()
        m.eval()
        s = C.encode_frame(m, entropy=bool(k & 1), segment=16)
        xq, _, cq, Lpre = C.unpack_frames_host([s], prev=state)[0]
        state = (xq, Lpre, cq)
        streams.append(s)
    _stream.append(streams)
    return streams


STREAM_VIEWS = [dict(size=(96, 160)), dict(size=(24, 40)), dict(crop=(8, 4, 40, 30)),
                dict(size=(90, 120), crop=(8, 4, 40, 30)), dict(size=(36, 100), crop=(10.25, 3.5, 20.5, 11.0))]


# --------------------------------------------------------------------------
# the sampling rule, restated

def axis(src, out, start, extent):
    """(xd float64 [out], owner pixel int64 [out], start table int64
    [tiles + 1]) of one axis, from the rule's text."""
    j = np.arange(out, dtype=np.float64)
    xd = start + ((2 * j + 1) * extent) / (2 * out) - 0.5
    p = np.clip(np.floor(xd + 0.5), 0, src - 1).astype(np.int64)
    tiles = (src + 15) // 16
    starts = np.array([(p >> 4 < t).sum() for t in range(tiles + 1)], dtype=np.int64)
    return xd, p, starts
