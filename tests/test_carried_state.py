"""The state the render and op paths carry from call to call -- counter parity,
a splat order sorted by an earlier call, a lazily copied M hint that picks
the composite kernel, cached shapes -- under inputs that CHANGE between calls
(tests/carried_cases.py).  The other suites repeat one input, so the order
always fits its frame, the hint is stale only in the harmless direction and
no shape changes mid-stream.

Three paths: ``op`` (gsplat.project_gaussians_2d + rasterize_gaussians_sum, the
C++ Functions of csrc/torch_ops.cpp, forward and backward), ``frame``
(render_frame_sum; ``bound``: BoundRender) and ``gop`` (render_frames_sum).
On every call:
  (a) the image equals the CPU oracle's on the pixels the oracle does not mark
      borderline (margin < 1e-5), rtol 1e-6 / atol 1e-5;
  (b) it is bit-equal to the image of the same model and shape earlier in the
      sequence, whatever order, parity or composite kernel either call got;
  (c) op: the gradients equal the oracle's (rtol 1e-4; atol 1e-4 max(H, W) / 2
      on means, 1e-3 on L, 1e-4 on colours);
  (d) gop: each frame is bit-equal to render_frame_sum of that frame alone.
Each sequence then shows, through the state window (_torch_ops.op_state, the
render paths' workspace attributes), that it reached the states it names.  No
sequence assumes a fresh workspace: torch hands streams out of a pool and the
workspaces are keyed by the raw handle, so all of them start from whatever
the tests before left.  Sequences 1-8 passed as the code stood; sequence 9 (a
model without splats between two frames) is the regression test of the one
carried-state bug they led to (frame.hip, see its test).

The CPU half (test_premises) pins what the sequences take for granted: every
model's density class against the kernels' thresholds, and the borderline
share (at most 0.1 % of a frame's pixels; the oracle gives 0-2 per frame).
"""
import numpy as np
import pytest
import torch

import carried_cases as C

REFRESH = 64     # torch_ops.cpp kOrderRefresh, train.ORDER_REFRESH_EVERY
PLAIN_PER_TILE = 8  # frame.hip kPlainProjMaxPerTile: at or below, the frame path skips its order


# --------------------------------------------------------------------------
# CPU: the premises

@pytest.mark.parametrize("name", ["alternation", "drift", "swings_same_n", "swings_changing_n",
                                  "shapes", "backward_pair", "two_streams", "no_splats",
                                  "gop"])
def test_premises(oracle, name):
    """Every distinct frame of the sequence, on the oracle alone: its density
    class is what its name says (M against 96 * tiles, the densest tile against
    256 and 1024) and at most 0.1 % of its pixels are borderline."""
    counts = []
    for s in C.distinct(C.all_steps()[name]):
        r = C.ref(s)
        C.check_class(s.model.kind, r)
        assert r.borderline <= C.borderline_cap(s.H, s.W), (s.model.name, r.borderline)
        counts.append(r.borderline)
    print(f"{name}: borderline pixels per distinct frame {counts}")
    if name == "gop":  # a list's class is its summed M against 96 * tiles * F
        thr = C.BANDED_PER_TILE * C.ntiles(C.BASE, C.BASE) * 4
        for models, _, kind in C.gop_lists():
            m = sum(C.ref(C.Step(x)).m for x in models)
            assert {"sparse": 0 < m < thr, "dense": m > thr, "empty": m == 0}[kind], (kind, m)
    if name == "drift":  # splats do walk in and out, and tiles cross the 256-entry slab
        ms = [C.ref(s).m for s in C.drift()]
        assert max(ms) > 1.3 * min(ms)
        tmax = [C.ref(s).tile_max for s in C.drift()]
        assert min(tmax) <= C.NARROW < max(tmax)


# --------------------------------------------------------------------------
# GPU: the paths

def T(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)  # (a copy: the models are read-only)


def N(t):
    return t.detach().cpu().numpy()


_on_dev = {}


def dev_model(m, dev):
    got = _on_dev.get(id(m))
    if got is None or got[0] is not m:
        got = _on_dev[id(m)] = (m, (T(m.means, dev), T(m.L, dev), T(m.colors, dev)))
    return got[1]


class Rec:
    def __init__(self, step, before, after, img, grads=None):
        self.step, self.before, self.after, self.img, self.grads = step, before, after, img, grads


class OpPath:
    """The drop-in operators on the default route (the C++ Functions)."""
    name, hwc = "op", True

    def __init__(self, dev):
        from gsvc_amd import _lib
        self.dev = dev
        self.ext = _lib.torch_ops()
        self.bg = torch.ones(3, device=dev)
        self.v = {}

    def state(self):
        return dict(self.ext.op_state(self.dev.index, torch.cuda.current_stream(self.dev).cuda_stream))

    def flags(self, before, step):
        """(ordered, refresh) of a call on ``step`` from the state ``before``
        (torch_ops.cpp slab_ws_ready + order_flags)."""
        n = step.model.n
        order_n = before["order_n"] if before["tiles"] == C.ntiles(step.H, step.W) else -1
        ordered = n > 0 and order_n == n
        return ordered, n > 0 and (not ordered or before["order_age"] + 1 >= REFRESH)

    def hint_used(self, rec):
        return rec.after["hint"]  # polled inside the call; nothing else changes it

    def forward(self, step):
        from gsplat.project_gaussians_2d import project_gaussians_2d
        from gsplat.rasterize_sum import rasterize_gaussians_sum
        H, W = step.H, step.W
        leaves = [t.detach().requires_grad_(True) for t in dev_model(step.model, self.dev)]
        m, l, c = leaves
        o = torch.ones(step.model.n, 1, device=self.dev)
        tb = ((W + 15) // 16, (H + 15) // 16, 1)
        xys, depths, radii, conics, nth = project_gaussians_2d(m, l, H, W, tb)
        out = rasterize_gaussians_sum(xys, depths, radii, conics, nth, c, o, H, W, 16, 16,
                                      background=self.bg)
        return out, leaves

    def v_out(self, H, W):
        if (H, W) not in self.v:
            self.v[(H, W)] = T(C.v_out(H, W), self.dev)
        return self.v[(H, W)]

    def call(self, step):
        out, leaves = self.forward(step)
        out.backward(self.v_out(step.H, step.W))
        return out.detach(), tuple(t.grad for t in leaves)


class FramePath:
    """render_frame_sum on activated inputs (no tanh, zero bound)."""
    name, hwc = "frame", False

    def __init__(self, dev):
        self.dev = dev
        self.bg = torch.ones(3, device=dev)
        self.bound = torch.zeros(3, device=dev)

    def ws(self):
        from gsvc_amd import render
        return render._workspaces.get((self.dev.index, render._raw_stream(self.dev.index)))

    def state(self):
        fw = self.ws()
        if fw is None:
            return dict(found=False, frame=0, hint=0, shape=None, hw=None, order_for=None,
                        order_age=0, dirty=True, cap=0)
        return dict(found=True, frame=fw.frame, hint=fw.hint.value, shape=fw.shape, hw=fw.hw,
                    order_for=fw.order_for, order_age=fw.order_age, dirty=fw.dirty,
                    cap=0 if fw.buf is None else fw.buf.numel())

    def flags(self, before, step):
        """render._workspace + train.order_flags; the kernel then skips the
        order while the hint is at or below 8 entries per tile (frame.hip)."""
        shape = (step.model.n, step.H, step.W)
        kept = not before["dirty"] and before["hw"] == shape[1:]
        ordered = kept and before["order_for"] == shape
        return ordered, not ordered or before["order_age"] + 1 >= REFRESH

    def hint_used(self, rec):
        return rec.before["hint"]

    def call(self, step):
        from gsvc_amd.render import render_frame_sum
        means, L, col = dev_model(step.model, self.dev)
        out = render_frame_sum(means, L, col, step.H, step.W, self.bg, xyz_tanh=False,
                               cholesky_bound=self.bound)
        return out[0], None


class BoundPath(FramePath):
    """BoundRender, one per model (it binds tensors and always applies tanh:
    the model's means2d are tanh of the bound xyz, see _tanh_pair)."""
    name = "bound"

    def __init__(self, dev):
        super().__init__(dev)
        self.renders = {}

    def call(self, step):
        from gsvc_amd.render import BoundRender
        b = self.renders.get(step.key)
        if b is None:
            _, L, col = dev_model(step.model, self.dev)
            b = self.renders[step.key] = BoundRender(step.model.xyz, L, col, step.H, step.W,
                                                     self.bg, cholesky_bound=self.bound)
        return b()[0], None


PATHS = {"op": OpPath, "frame": FramePath, "bound": BoundPath}


def run(path, steps, recs, sync_at=()):
    for k, s in enumerate(steps):
        if k in sync_at:
            torch.cuda.synchronize()
        before = path.state()
        img, grads = path.call(s)
        recs.append(Rec(s, before, path.state(), img, grads))
    return recs


def check(path, recs):
    """(a), (b) and (c) on every recorded call."""
    torch.cuda.synchronize()
    first = {}
    for i, r in enumerate(recs):
        s = r.step
        ref = C.ref(s)
        what = f"{path.name} call {i} ({s.model.name} {s.H}x{s.W})"
        want = ref.out if path.hwc else ref.planes
        ok = np.broadcast_to(ref.ok[..., None] if path.hwc else ref.ok[None], want.shape)
        got = N(r.img)
        assert got.shape == want.shape, what
        np.testing.assert_allclose(got[ok], want[ok], rtol=1e-6, atol=1e-5, err_msg=what)
        f = first.setdefault(s.key, (i, r))
        if f[1] is not r:
            assert torch.equal(r.img, f[1].img), f"{what}: not the bits of call {f[0]}"
        if r.grads is not None:
            check_grads(r.grads, ref, what)


def check_grads(grads, ref, what):
    v_mean, v_L, v_rgb = ref.grads()
    scale = max(ref.H, ref.W) / 2
    np.testing.assert_allclose(N(grads[0]), v_mean, rtol=1e-4, atol=1e-4 * scale, err_msg=what + " means")
    np.testing.assert_allclose(N(grads[1]), v_L, rtol=1e-4, atol=1e-3, err_msg=what + " L")
    np.testing.assert_allclose(N(grads[2]), v_rgb, rtol=1e-4, atol=1e-4, err_msg=what + " colours")


def dense_hint(hint, H=C.BASE, W=C.BASE, frames=1):
    """raster_sum.hip sum_forward_dense: the banded composite."""
    return hint > C.BANDED_PER_TILE * C.ntiles(H, W) * frames


def uses_order(path, rec):
    """The call inserted its ids through an order sorted by an earlier call."""
    if not path.flags(rec.before, rec.step)[0]:
        return False
    if path.hwc:
        return rec.before["order_n"] == rec.step.model.n
    return path.hint_used(rec) > PLAIN_PER_TILE * C.ntiles(rec.step.H, rec.step.W)


def check_refresh_bookkeeping(path, recs):
    """A refresh resets the age, an ordered call adds one to it; returns the
    indices of the refreshes that the age brought about."""
    wraps = []
    for i, r in enumerate(recs):
        ordered, refresh = path.flags(r.before, r.step)
        if refresh:
            assert r.after["order_age"] == 0, i
            if ordered:
                assert r.before["order_age"] == REFRESH - 1, i
                wraps.append(i)
        elif ordered:
            assert r.after["order_age"] == r.before["order_age"] + 1, i
        if path.hwc and r.step.model.n > 0:
            assert r.after["order_n"] == r.step.model.n, i
            assert r.after["calls"] == (r.before["calls"] + 1
                                        if r.before["tiles"] == r.after["tiles"] else 1), i
    return wraps


def _tanh_pair(dev):
    """The alternation's two models as BoundRender takes them: xyz = atanh of
    the means, and the model's means2d the device's own tanh of it (the
    kernel's tanhf is torch.tanh bit for bit, test_gpu_sync_free), so the
    oracle renders the positions the kernel does."""
    steps = C.alternation()
    pair = {}
    for s in steps:
        if id(s.model) not in pair:
            m = s.model
            xyz = T(np.arctanh(m.means.astype(np.float64)).astype(np.float32), dev)
            t = C.Model(m.name + "_tanh", N(torch.tanh(xyz)), m.L, m.colors, m.kind)
            t.xyz = xyz
            pair[id(m)] = t
            r = C.ref(C.Step(t))
            C.check_class(t.kind, r)
            assert r.borderline <= C.borderline_cap(C.BASE, C.BASE)
    return [C.Step(pair[id(s.model)]) for s in steps]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["op", "frame", "bound"])
def test_equal_n_alternation(cuda, oracle, name):
    """1, the K-frame detector's pattern: two dense256 models of equal N
    alternate on one stream for 132 calls.  Shown through the state: the age
    wrapped into a refresh at least once on EACH model, and each model ran
    ordered calls (order_n == n; frame paths: with the hint above the plain
    projection's bar) after the latest refresh had sorted the OTHER model."""
    path = PATHS[name](cuda)
    steps = _tanh_pair(cuda) if name == "bound" else C.alternation()
    recs = run(path, steps, [])
    check(path, recs)
    if name == "bound":  # BoundRender is render_frame_sum of the same tensors
        from gsvc_amd.render import render_frame_sum
        for s in C.distinct(steps):
            _, L, col = dev_model(s.model, cuda)
            again = render_frame_sum(s.model.xyz, L, col, s.H, s.W, path.bg, xyz_tanh=True,
                                     cholesky_bound=path.bound)[0]
            assert torch.equal(again, next(r.img for r in recs if r.step.key == s.key))
    wraps = check_refresh_bookkeeping(path, recs)
    a, b = (s.model for s in C.distinct(steps))
    assert {id(recs[i].step.model) for i in wraps} == {id(a), id(b)}, wraps
    sorted_for, crossed = None, set()
    for r in recs:
        if path.flags(r.before, r.step)[1]:
            sorted_for = r.step.model
        elif sorted_for is not None and sorted_for is not r.step.model and uses_order(path, r):
            crossed.add(id(r.step.model))
    assert crossed == {id(a), id(b)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["op", "frame"])
def test_drift(cuda, oracle, name):
    """2, training-like motion: every call moves every splat (a tenth walk in
    from off-screen, a tenth walk out) and rescales L; the oracle checks each
    of the 70 calls, and a last call repeats call 0's inputs bit for bit.
    Shown: the order stayed valid by N throughout, most calls used an order
    sorted for earlier positions, and the age wrapped into a refresh."""
    path = PATHS[name](cuda)
    recs = run(path, C.drift(), [])
    check(path, recs)
    assert recs[-1].step.key == recs[0].step.key
    wraps = check_refresh_bookkeeping(path, recs)
    assert wraps
    # (the frame path's hint may take 32 calls to pass the plain projection's bar)
    assert sum(uses_order(path, r) and not path.flags(r.before, r.step)[1] for r in recs) >= 20


def _run_phases(path, phases):
    """Each phase without a host wait but one before its call 16 (the hint's
    copy has then landed), and one between phases."""
    out = []
    for steps in phases:
        torch.cuda.synchronize()
        out.append(run(path, steps, [], sync_at=(16,)))
    return out


def _check_hint_turnover(path, per_phase):
    """The first call of a phase ran on the previous phase's hint -- the wrong
    kernel when the class changed -- and its last call on its own."""
    stale_high = stale_low = 0
    for k, recs in enumerate(per_phase):
        want = C.ref(recs[0].step).m
        assert dense_hint(path.hint_used(recs[-1])) == dense_hint(want), k
        assert path.hint_used(recs[-1]) == want, k
        if k:
            before = C.ref(per_phase[k - 1][0].step).m
            assert path.hint_used(recs[0]) == before, k
            stale_high += dense_hint(before) and not dense_hint(want)
            stale_low += dense_hint(want) and not dense_hint(before)
    return stale_high, stale_low


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["op", "frame"])
def test_density_swings_same_n(cuda, oracle, name):
    """3: one 3000-splat model through sparse -> dense1024 -> empty -> dense256
    -> sparse, 34 constant calls per phase; only the means and the L scale
    change, so the order is kept across every swing.  Shown: each phase began
    on the previous phase's hint (the sparse composite on tiles past 1024
    entries, the banded one on an empty and on a sparse frame) and ended on
    its own, and (b) held across the switch; the order was never dropped."""
    path = PATHS[name](cuda)
    per_phase = _run_phases(path, C.swings_same_n())
    recs = [r for p in per_phase for r in p]
    check(path, recs)
    high, low = _check_hint_turnover(path, per_phase)
    assert high >= 2 and low >= 2
    check_refresh_bookkeeping(path, recs)
    for r in recs[1:]:  # same N, same shape: ordered from the second call on
        assert path.flags(r.before, r.step)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["op", "frame"])
def test_density_swings_changing_n(cuda, oracle, name):
    """4: the same classes with N changing (300 -> 3000 -> 1500 off-screen ->
    3000 -> 300).  Shown: the first call of each phase dropped the order and
    refreshed (the order buffer is reused when N shrinks), the rest ran
    ordered, and the hint turned over as in 3."""
    path = PATHS[name](cuda)
    per_phase = _run_phases(path, C.swings_changing_n())
    recs = [r for p in per_phase for r in p]
    check(path, recs)
    high, low = _check_hint_turnover(path, per_phase)
    assert high >= 2 and low >= 2
    check_refresh_bookkeeping(path, recs)
    for k, p in enumerate(per_phase):
        if k:
            assert path.flags(p[0].before, p[0].step) == (False, True), k
        for r in p[1:]:
            assert path.flags(r.before, r.step)[0], k


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["op", "frame"])
def test_shape_changes(cuda, oracle, name):
    """5: prune, densify, 60 x 100 then 100 x 60 (both 28 tiles, tbx 7 and 4),
    one splat, a ragged shape and back, three calls each so both parities meet
    each shape.  Shown: the op path kept its counters (tiles == 28, calls
    counting on) and its order across the 60 x 100 / 100 x 60 step; the frame
    path restarted its frame count there and whenever (H, W) changed, and only
    then."""
    path = PATHS[name](cuda)
    per_step = [run(path, steps, []) for steps in C.shapes()]
    recs = [r for p in per_step for r in p]
    check(path, recs)
    check_refresh_bookkeeping(path, recs)
    wide, tall = per_step[3], per_step[4]
    assert (wide[0].step.H, wide[0].step.W, tall[0].step.H, tall[0].step.W) == (60, 100, 100, 60)
    if name == "op":
        assert wide[-1].after["tiles"] == tall[0].after["tiles"] == 28
        assert tall[0].after["calls"] == wide[-1].after["calls"] + 1
        assert path.flags(tall[0].before, tall[0].step)[0] and uses_order(path, tall[0])
        for p in per_step:  # both parities of the slab counters
            assert {r.after["calls"] & 1 for r in p} == {0, 1}
    else:
        for k, p in enumerate(per_step):
            r = p[0]
            # re-zeroed (frame count restarted) when (H, W) changed or the buffer grew
            rezeroed = r.before["hw"] != (r.step.H, r.step.W) or r.before["cap"] != r.after["cap"]
            assert r.after["frame"] == (1 if rezeroed else r.before["frame"] + 1), k
            assert r.after["shape"] == (r.step.model.n, r.step.H, r.step.W)
            assert {x.after["frame"] & 1 for x in p} == {0, 1}
        assert tall[0].before["hw"] == (60, 100) and tall[0].after["frame"] == 1


@pytest.mark.gpu
def test_backward_after_other_forwards(cuda, oracle):
    """6 (op): forward A, forward B (same N, same stream, so B's forward reuses
    the counters and the order A's used), then backward A, backward B; and
    forward A kept with retain_graph, forward B, backward A twice -- the
    second backward gives the same gradients, not doubled."""
    path = OpPath(cuda)
    sa, sb = C.backward_pair()
    path.call(sa)  # whatever came before, the order is now sorted for this N
    out_a, la = path.forward(sa)
    st = path.state()
    assert st["order_n"] == sa.model.n == sb.model.n
    out_b, lb = path.forward(sb)
    assert path.state()["calls"] == st["calls"] + 1
    v = path.v_out(sa.H, sa.W)
    out_a.backward(v)
    out_b.backward(v)
    torch.cuda.synchronize()
    check_grads([t.grad for t in la], C.ref(sa), "backward A after forward B")
    check_grads([t.grad for t in lb], C.ref(sb), "backward B after backward A")

    out_a, la = path.forward(sa)
    out_b, _ = path.forward(sb)
    out_a.backward(v, retain_graph=True)
    first = [t.grad.clone() for t in la]
    for t in la:
        t.grad = None
    out_a.backward(v)
    torch.cuda.synchronize()
    check_grads(first, C.ref(sa), "first backward of a retained graph")
    check_grads([t.grad for t in la], C.ref(sa), "second backward of a retained graph")
    recs = [Rec(sa, None, None, out_a.detach()), Rec(sb, None, None, out_b.detach())]
    check(path, recs)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["op", "frame"])
def test_two_streams(cuda, oracle, name):
    """7: dense1024 on one stream, sparse on another, 40 calls taking turns
    (the turn order swaps at call 17, so the op path's device-wide hint copy,
    every 16th call, lands on both).  Shown (op): the dense model ran on the
    sparse model's hint and the sparse model on the dense one's, each stream
    keeping its own counters and order; (frame): one workspace per stream."""
    path = PATHS[name](cuda)
    sa, sb = C.two_streams()
    for s in (sa, sb):
        dev_model(s.model, cuda)
    path.call(sa)  # (the op path's v_out, uploaded on the default stream)
    torch.cuda.synchronize()
    streams = (torch.cuda.Stream(cuda), torch.cuda.Stream(cuda))
    assert streams[0].cuda_stream != streams[1].cuda_stream
    recs = []
    for i in range(40):
        if i % 4 == 0:
            torch.cuda.synchronize()
        which = (i + (i >= 17)) % 2
        with torch.cuda.stream(streams[which]):
            run(path, [(sa, sb)[which]], recs)
    check(path, recs)
    ra = [r for r in recs if r.step is sa]
    rb = [r for r in recs if r.step is sb]
    if name == "op":
        assert any(not dense_hint(path.hint_used(r)) for r in ra)
        assert any(dense_hint(path.hint_used(r)) for r in rb)
        for rs in (ra, rb):  # per stream: its own call count and order
            assert all(y.after["calls"] == x.after["calls"] + 1 for x, y in zip(rs, rs[1:]))
            assert all(r.after["order_n"] == r.step.model.n for r in rs)
    else:
        assert all(r.after["shape"] == (r.step.model.n, C.BASE, C.BASE) for r in recs)
        assert all(y.after["frame"] == x.after["frame"] + 1 for x, y in zip(ra, ra[1:]))
        assert all(y.after["frame"] == x.after["frame"] + 1 for x, y in zip(rb, rb[1:]))


@pytest.mark.gpu
def test_frame_without_splats_then_empty_frame(cuda, oracle):
    """9 (frame): render_frame_sum of a model with NO splats between a frame
    with intersections and one whose splats are all off-screen.  The call
    without splats launches no projection, so nothing cleared the other
    parity's M slot: the off-screen frame then added its 0 to the first
    frame's M, took the M >= 1 branch and came out black instead of the
    background (fixed in frame.hip: that call now zeroes both slots)."""
    path = FramePath(cuda)
    recs = run(path, C.no_splats(), [])
    check(path, recs)
    assert [C.ref(r.step).m > 0 for r in recs] == [True, False, False] * 2 + [True]
    assert {r.before["frame"] & 1 for r in recs if r.step.model.n == 0} == {0, 1}
    assert float(recs[2].img.min()) == 1.0  # the background


@pytest.mark.gpu
def test_gop_lists(cuda, oracle):
    """8 (gop): F = 4 at 64 x 64 through one workspace key: sparse, mixed
    (dense1024, one splat, none, sparse), all empty, dense1024, sparse -- 18
    calls each -- then lists whose total N shrinks and grows.  Each frame
    against the oracle and bit-equal to render_frame_sum of it alone.  Shown:
    the key stayed (4, 64, 64); each 18-call list began on the previous
    list's summed M and ended on its own, so sparse lists ran banded and
    dense lists sparse; the later lists changed N with the call count running
    on (no re-zero)."""
    from gsvc_amd import render
    from gsvc_amd.render import render_frames_sum
    frame_path = FramePath(cuda)
    H = W = C.BASE
    lists = C.gop_lists()
    single = {}
    for models, _, _ in lists:
        for m in models:
            if id(m) not in single:
                single[id(m)] = Rec(C.Step(m), None, None, frame_path.call(C.Step(m))[0])
    check(frame_path, list(single.values()))
    key = (cuda.index, torch.cuda.current_stream(cuda).cuda_stream)
    hints, runs = [], []
    # the largest list once first (checked like the rest): the workspace then
    # never has to grow, which would re-zero it and restart its call count
    for models, calls, kind in [(lists[3][0], 1, "dense")] + lists:
        parts = [dev_model(m, cuda) for m in models]
        xyz, chol, feat = (torch.cat([p[j] for p in parts]).contiguous() for j in range(3))
        sizes = [m.n for m in models]
        torch.cuda.synchronize()
        outs, used, counts = [], [], []
        for k in range(calls):
            if k == 16:
                torch.cuda.synchronize()
            bw = render._batch_workspaces.get(key)
            used.append(bw.hint if bw is not None and bw.key == (4, H, W) else 0)
            outs.append(render_frames_sum(xyz, chol, feat, sizes, H, W, frame_path.bg,
                                          xyz_tanh=False, cholesky_bound=frame_path.bound))
            bw = render._batch_workspaces[key]
            assert bw.key == (4, H, W)
            counts.append(bw.call)
        torch.cuda.synchronize()
        for k, out in enumerate(outs):
            assert out.shape == (4, 3, H, W)
            for b, m in enumerate(models):
                ref = C.ref(C.Step(m))
                what = f"list {sizes} call {k} frame {b}"
                ok = np.broadcast_to(ref.ok[None], ref.planes.shape)
                np.testing.assert_allclose(N(out[b])[ok], ref.planes[ok], rtol=1e-6, atol=1e-5,
                                           err_msg=what)
                assert torch.equal(out[b], single[id(m)].img), what
        hints.append(used)
        runs.append(counts)
    hints, runs = hints[1:], runs[1:]
    thr = lambda h: dense_hint(h, H, W, 4)  # noqa: E731
    total = [sum(C.ref(C.Step(m)).m for m in models) for models, _, _ in lists]
    for k in range(5):
        assert hints[k][-1] == total[k], k
        if k:
            assert hints[k][0] == total[k - 1], k
    assert thr(hints[1][0]) is False and thr(hints[3][0]) is False  # dense lists, sparse kernel
    assert thr(hints[2][0]) is True and thr(hints[4][0]) is True    # empty / sparse lists, banded
    flat = [c for counts in runs[4:] for c in counts]
    assert all(y == x + 1 for x, y in zip(flat, flat[1:]))
    assert {c & 1 for c in runs[5]} == {0, 1} and {c & 1 for c in runs[6]} == {0, 1}
