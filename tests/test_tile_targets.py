"""The training tile kernel's target loads and candidate-id load (train.hip,
train_tile_band_kernel).

Targets: with ``img_w % 4 == 0`` and a 16-byte aligned ``gt`` the tile's
targets arrive as three 16-byte loads per tile from wave 1, laid out
[c][16 rows][16 px]; any other width or alignment keeps the 4-byte pair loads.
Both paths feed the same arithmetic, so the same target values passed aligned
and at a one-float storage offset must give the same bits -- loss words, clamped
render, gradients, and whole carried trajectories -- at full, partial and
one-row edge tiles and through every order path (<= 64 entries, the bitmap sort,
more than 256).  The targets are random in [-0.2, 1.2]: distinct at every pixel
and channel, with values outside the clamp, so a misplaced target changes the
loss, which is also held to the float64 loss of the call's own render.

Candidate ids: wave 0 loads all 64 ids of a sparse carried tile in its first
round trip; 32, 33, 50, 64 and 65 splats on one tile are the two ends of lanes
32-63 and one count inside, carried against re-projected bins.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture
def deterministic():
    prev = torch.are_deterministic_algorithms_enabled()
    prev_warn = torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    yield
    torch.use_deterministic_algorithms(prev, warn_only=prev_warn)


def _targets(H, W, dev, seed=7):
    """The same [1, 3, H, W] values twice: 16-byte aligned, and as a contiguous
    view one float into its storage."""
    g = torch.Generator().manual_seed(seed)
    vals = (torch.rand(3 * H * W, generator=g) * 1.4 - 0.2).to(dev)
    aligned = vals.clone().view(1, 3, H, W)
    buf = torch.empty(3 * H * W + 8, device=dev)
    buf[1:1 + 3 * H * W] = vals
    off = buf[1:1 + 3 * H * W].view(1, 3, H, W)
    assert aligned.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 4
    assert off.is_contiguous() and torch.equal(aligned, off)
    return aligned, off


def _step(m, gt, loss_type):
    from gsvc_amd.train import train_step_sum
    n, H, W = m._xyz.shape[0], m.H, m.W
    g = torch.empty((n, 9), device=gt.device)
    render = torch.empty((1, 3, H, W), device=gt.device)
    losses = train_step_sum(m._xyz.data, m._cholesky.data, m._features_dc.data, m.rgb_W.data, False,
                            m.cholesky_bound, m.background, gt, H, W, loss_type, render_out=render,
                            grads_out=g)
    torch.cuda.synchronize()
    return losses, render, g


def _loss_is_the_renders(losses, render, gt):
    d = render.double() - gt.double()
    torch.testing.assert_close(losses[0].double(), (d * d).mean(), rtol=1e-5, atol=0.0)
    torch.testing.assert_close(losses[1].double(), d.abs().mean(), rtol=1e-5, atol=0.0)


def _both_alignments(cuda, H, W, n, loss_type, grads):
    from gsvc_amd.frame import make_frame_model
    m = make_frame_model(H, W, n, cuda, seed=n + 5)
    aligned, off = _targets(H, W, cuda)
    la, ra, ga = _step(m, aligned, loss_type)
    lo, ro, go = _step(m, off, loss_type)
    print(f"{H}x{W} n={n} {loss_type}: aligned {la.tolist()} offset {lo.tolist()}")
    assert torch.equal(la, lo)
    assert torch.equal(ra, ro)
    if grads:
        assert torch.equal(ga, go)
    _loss_is_the_renders(la, ra, aligned)
    _loss_is_the_renders(lo, ro, off)
    assert float(la[0]) > 0.0 and bool(ga.abs().sum() > 0)


SHAPES = [(16, 16, 40),    # one full tile
          (20, 36, 60),    # partial bottom tile of 4 rows, partial right tile of 4 px, W % 16 != 0
          (24, 48, 60),    # bottom tile of exactly one band
          (17, 32, 40),    # one image row in the last tile row
          (16, 16, 100),   # more than 64 entries: the bitmap sort, both waves in the order
          (16, 16, 400)]   # more than 256 entries


@pytest.mark.parametrize("H,W,n", SHAPES)
@pytest.mark.parametrize("loss_type", ["L2", "L1"])
def test_aligned_and_offset_targets_deterministic(cuda, deterministic, H, W, n, loss_type):
    _both_alignments(cuda, H, W, n, loss_type, grads=True)


@pytest.mark.parametrize("H,W,n", SHAPES)
@pytest.mark.parametrize("loss_type", ["L2", "L1"])
def test_aligned_and_offset_targets_atomic(cuda, H, W, n, loss_type):
    assert not torch.are_deterministic_algorithms_enabled()
    _both_alignments(cuda, H, W, n, loss_type, grads=False)


@pytest.mark.parametrize("H,W,n", [(18, 34, 40), (16, 17, 20)])
@pytest.mark.parametrize("loss_type", ["L2", "L1"])
def test_widths_of_partial_groups_take_the_pair_loads(cuda, deterministic, H, W, n, loss_type):
    """W % 4 != 0: the 4-byte loads whatever the alignment."""
    _both_alignments(cuda, H, W, n, loss_type, grads=True)


def _run(cuda, H, W, n, steps, gt, carry=True):
    from gsvc_amd import train as T
    from gsvc_amd.frame import make_frame_model
    old = T.CARRY_BINS
    T.CARRY_BINS = carry
    try:
        m = make_frame_model(H, W, n, cuda, seed=3)
        losses = [float(m.train_iter(gt, it)[0]) for it in range(1, steps + 1)]
        torch.cuda.synchronize()
        assert m.fused_steps == steps
        return m, losses
    finally:
        T.CARRY_BINS = old


def _same(a, b):
    la, lb = a[1], b[1]
    assert la == lb
    ma, mb = a[0], b[0]
    for k, v in ma.state_dict().items():
        assert torch.equal(v, mb.state_dict()[k]), k
    for p, q in zip(ma.optimizer.param_groups[0]["params"], mb.optimizer.param_groups[0]["params"]):
        for key in ("exp_avg", "exp_avg_sq", "exp_avg_diff", "neg_pre_grad"):
            assert torch.equal(ma.optimizer.state[p][key], mb.optimizer.state[q][key]), key


def test_carried_steps_aligned_equal_offset(cuda, deterministic):
    aligned, off = _targets(20, 36, cuda)
    a = _run(cuda, 20, 36, 60, 5, aligned)
    b = _run(cuda, 20, 36, 60, 5, off)
    print("losses", a[1], b[1])
    _same(a, b)


@pytest.mark.parametrize("n", [32, 33, 50, 64, 65])
def test_candidate_ids_carried_equal_reprojected(cuda, deterministic, n):
    from gsvc_amd.frame import synthetic_gt
    gt = synthetic_gt(16, 16, 4, cuda)
    a = _run(cuda, 16, 16, n, 4, gt, carry=True)
    b = _run(cuda, 16, 16, n, 4, gt, carry=False)
    print("losses", a[1], b[1])
    _same(a, b)
