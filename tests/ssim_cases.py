"""Cases, references and error measures shared by test_ssim_edges.py (the HIP
kernels) and tests/analysis/ssim_bars.py (the fp32 restatement on the CPU, from
which the bars come).  The references import nothing from the code under test:
values are the float64 oracle's, gradients are CPU float64 autograd through the
torch restatement of test_ssim.py."""
import numpy as np
import torch
import torch.nn.functional as F

from test_ssim import _pair, _t_gauss, _t_terms, t_ms_ssim, t_ssim

DEFAULT_WEIGHTS = [0.0448, 0.2856, 0.3001, 0.2363, 0.1333]
W8 = [.05, .1, .15, .2, .2, .15, .1, .05]


def case(id, kind, shape, family=None, seed=11, anti=False, warns=0, **opts):
    """kind: 'ssim' or 'ms'.  opts: the keyword arguments of the call besides
    size_average (data_range defaults to 1).  warns: how many "Skipping Gaussian
    Smoothing" warnings the call raises.  anti: Y[:, 0] = 1 - X[:, 0]."""
    opts.setdefault("data_range", 1)
    fam = family or kind
    return dict(id=id, kind=kind, shape=shape, family=fam, seed=seed, anti=anti, warns=warns,
                opts=opts)


# -- SSIM, data_range 1
SSIM_CASES = [
    # window 11 on the edges of the 16x64 output tiles (Ho = H - 10, Wo = W - 10)
    # and of the 16x64 input tiles of the gradient kernel
    case("t-26x73", "ssim", (2, 3, 26, 73)),     # Wo 63
    case("t-26x74", "ssim", (2, 3, 26, 74)),     # Ho 16, Wo 64
    case("t-27x75", "ssim", (2, 3, 27, 75)),     # Ho 17, Wo 65
    case("t-16x64", "ssim", (1, 3, 16, 64)),     # one input tile
    case("t-17x65", "ssim", (1, 3, 17, 65)),
    case("t-33x129", "ssim", (1, 2, 33, 129)),
    case("t-32x128", "ssim", (1, 3, 32, 128)),
    # the other accepted windows (the t < kv / t < kh paths of the unrolled loops)
    case("w1", "ssim", (1, 3, 43, 139), win_size=1),
    case("w3", "ssim", (1, 3, 43, 139), win_size=3),
    case("w7", "ssim", (1, 3, 43, 139), win_size=7),
    case("w9", "ssim", (1, 3, 43, 139), win_size=9),
    case("w7-22x70", "ssim", (1, 2, 22, 70), win_size=7),   # Ho 16, Wo 64
    case("w7-23x71", "ssim", (1, 2, 23, 71), win_size=7),   # Ho 17, Wo 65
    case("w1-20x30", "ssim", (1, 1, 20, 30), win_size=1),
    # dimensions shorter than or equal to the window
    case("s-40x7", "ssim", (1, 2, 40, 7), warns=1),          # kh = 1, kv = 11
    case("s-5x9", "ssim", (1, 2, 5, 9), warns=2),            # identity both ways
    case("s-11x11", "ssim", (1, 2, 11, 11)),                 # Ho = Wo = 1
    case("s-11x80", "ssim", (1, 2, 11, 80)),                 # Ho = 1
    case("s-30x11", "ssim", (1, 2, 30, 11)),                 # Wo = 1
    # more than 256 planes: the stride loop of the one-block combine kernel
    case("p270", "ssim", (90, 3, 12, 13)),
    # options
    case("K", "ssim", (2, 3, 27, 75), K=(0.02, 0.05)),
    case("sig0.8", "ssim", (2, 3, 27, 75), win_sigma=0.8),
    case("sig2.5", "ssim", (2, 3, 27, 75), win_sigma=2.5),
    # anti-correlated channel 0, no clamp: its gradient is not zero
    case("anti", "ssim", (2, 3, 176, 200), anti=True),
    case("anti-nonneg", "ssim", (2, 3, 176, 200), anti=True, nonnegative_ssim=True),
]

# -- MS-SSIM, data_range 1
MS_CASES = [
    case("m-162x200", "ms", (1, 3, 162, 200)),   # 162 81 41 21 11 x 200 100 50 25 13
    case("m-161x203", "ms", (1, 3, 161, 203)),
    case("m-w3", "ms", (2, 2, 65, 49), win_size=3),
    case("m-w3-K-sig", "ms", (2, 2, 65, 49), win_size=3, K=(0.02, 0.05), win_sigma=0.8),
    case("m-w7", "ms", (1, 3, 113, 139), win_size=7),
    case("m-L1", "ms", (2, 2, 65, 49), win_size=3, weights=[0.7]),
    case("m-L2", "ms", (2, 2, 65, 49), win_size=3, weights=[0.4, 0.6]),
    case("m-L3", "ms", (2, 2, 65, 49), win_size=3, weights=[0.2, 0.3, 0.5]),
    # 40 20 10 5 3 2 1 1 x 52 26 13 7 4 2 1 1: the last levels are not filtered
    case("m-L8", "ms", (1, 2, 40, 52), win_size=3, weights=W8),
    # anti-correlated channel 0: its cs is negative at levels 0..2 (-0.99, -0.95,
    # -0.82), then C2 takes over (level 3: -0.40 / -0.48; the last level's ssim
    # is +0.32 / +0.41 -- a positive term beside clamped ones in the 5-level case)
    case("m-anti3", "ms", (2, 3, 176, 200), anti=True, weights=[0.2, 0.3, 0.5]),
    case("m-anti", "ms", (2, 3, 176, 200), anti=True),
]

# -- data_range 255 on 255 X, 255 Y: E[x^2] - mu^2 cancels at 255^2
R255_CASES = [
    case("r255-ssim", "ssim", (1, 3, 27, 75), family="r255", data_range=255),
    case("r255-ms", "ms", (1, 3, 161, 203), family="r255", data_range=255),
]

CASES = SSIM_CASES + MS_CASES + R255_CASES
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)

# the planes that clamp, per case id (every other case: none); asserted on the
# float64 reference before anything is compared
CLAMPED = {"anti-nonneg": [(0, 0), (1, 0)], "m-anti3": [(0, 0), (1, 0)], "m-anti": [(0, 0), (1, 0)]}
# how far every raw per-plane term of those inputs stays from the relu kink:
# case id -> (a, b), every term <= a or >= b.  fp32 moves a term by 1e-6, so
# either margin is five orders wide.  The 5-level case cannot have a = -0.5 (its
# level-3 cs, above); it keeps the positive side's distance on both sides.
KINK = {"anti": (-0.5, 0.3), "anti-nonneg": (-0.5, 0.3), "m-anti3": (-0.5, 0.3),
        "m-anti": (-0.3, 0.3)}


def inputs(c):
    """(X, Y) fp32 CPU tensors of the case, scaled to its data_range."""
    X, Y = _pair(c["shape"], c["seed"])
    if c["anti"]:
        Y = Y.clone()
        Y[:, 0] = 1 - X[:, 0]
    r = c["opts"]["data_range"]
    return (X * r, Y * r) if r != 1 else (X, Y)


def upstream(B, dtype=torch.float64):
    return torch.linspace(0.5, 1.5, B, dtype=dtype)


def raw_terms(c, X, Y, win_dtype):
    """The per-plane terms before relu: [levels, B, C] (SSIM: one level, the
    mean ssim_map; MS-SSIM: mean cs per level, mean ssim_map at the last)."""
    o = c["opts"]
    r, K = o["data_range"], o.get("K", (0.01, 0.03))
    C1, C2 = (K[0] * r) ** 2, (K[1] * r) ** 2
    win = _t_gauss(o.get("win_size", 11), o.get("win_sigma", 1.5), win_dtype)
    if c["kind"] == "ssim":
        return _t_terms(X, Y, win, C1, C2)[0][None]
    n = len(o.get("weights") or DEFAULT_WEIGHTS)
    raw = []
    for i in range(n):
        s, cs = _t_terms(X, Y, win, C1, C2)
        raw.append(cs if i < n - 1 else s)
        if i < n - 1:
            pad = [s_ % 2 for s_ in X.shape[2:]]
            X = F.avg_pool2d(X, kernel_size=2, padding=pad)
            Y = F.avg_pool2d(Y, kernel_size=2, padding=pad)
    return torch.stack(raw)


def plane_values(c, raw):
    """Per-plane values [B, C] from the raw terms with relu'(0) = 0: a plane
    with a clamped level is 0 and is left out of the graph (0 ** (w - 1) times
    relu' would put a NaN into autograd).  Returns (values, clamped mask)."""
    o = c["opts"]
    if c["kind"] == "ssim":
        clamp = (raw[0] <= 0) if o.get("nonnegative_ssim") else torch.zeros_like(raw[0], dtype=torch.bool)
        w = raw.new_ones(1)
    else:
        clamp = (raw <= 0).any(0)
        w = raw.new_tensor(o.get("weights") or DEFAULT_WEIGHTS)
    vals = torch.zeros_like(raw[0])
    keep = ~clamp
    if c["kind"] == "ssim":
        vals[keep] = raw[0][keep]
    else:
        vals[keep] = torch.prod(raw[:, keep] ** w.view(-1, 1), dim=0)
    return vals, clamp


def reference(c, avg=False, dtype=torch.float64, want=(True, True)):
    """CPU reference in `dtype` (float64: the reference; float32: the restatement
    whose error sets the bars): the value ([B], or a scalar when avg), dX, dY for
    the upstream linspace(0.5, 1.5, B) (1 when avg), the raw terms and the
    clamped-plane mask.  want: which of X, Y require a gradient."""
    X, Y = inputs(c)
    X = X.to(dtype).requires_grad_(want[0])
    Y = Y.to(dtype).requires_grad_(want[1])
    raw = raw_terms(c, X, Y, dtype)
    vals, clamp = plane_values(c, raw)
    out = vals.mean() if avg else vals.mean(1)
    loss = out if avg else (out * upstream(out.numel(), dtype)).sum()
    loss.backward()
    return dict(value=out.detach(), dX=X.grad, dY=Y.grad, raw=raw.detach(), clamped=clamp)


def library_reference(c, avg=False):
    """The same value and gradients through t_ssim / t_ms_ssim in float64 (torch's
    own relu): what `reference` must equal wherever no plane clamps."""
    X, Y = inputs(c)
    X, Y = X.double().requires_grad_(True), Y.double().requires_grad_(True)
    o = dict(c["opts"])
    fn = t_ssim if c["kind"] == "ssim" else t_ms_ssim
    out = fn(X, Y, size_average=avg, win_dtype=torch.float64, **o)
    (out if avg else (out * upstream(out.numel())).sum()).backward()
    return out.detach(), X.grad, Y.grad


def oracle_value(oracle, c, avg=False):
    X, Y = inputs(c)
    o = dict(c["opts"])
    fn = oracle.ssim if c["kind"] == "ssim" else oracle.ms_ssim
    return np.asarray(fn(X.numpy(), Y.numpy(), size_average=avg, **o), np.float64)


def band_mask(shape, win_size):
    """The outer band of width win_size - 1 of every plane (the whole plane
    where it is narrower than two bands; everything for win_size 1 would be
    empty, so the band is then one pixel wide)."""
    b = max(win_size - 1, 1)
    m = torch.ones(shape[-2:], dtype=torch.bool)
    if shape[-2] > 2 * b and shape[-1] > 2 * b:
        m[b:-b, b:-b] = False
    return m


def grad_errors(got, ref, win_size, planes=None):
    """(whole, band): the largest |got - ref| over the tensor relative to the
    reference's largest element, and over the outer band relative to the
    band's largest reference element.  planes: a [B, C] mask of the planes to
    look at (default all)."""
    got, ref = got.double().cpu(), ref.double().cpu()
    if planes is not None:
        got, ref = got[planes], ref[planes]
    m = band_mask(ref.shape, win_size)
    d = (got - ref).abs()
    whole = float(d.max()) / float(ref.abs().max())
    band = float(d[..., m].max()) / float(ref[..., m].abs().max())
    return whole, band
