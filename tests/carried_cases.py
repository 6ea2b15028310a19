"""Inputs and the CPU reference shared by test_carried_state.py's premise tests
(CPU) and sequences (GPU).  No GPU code: models are numpy arrays (means2d, L,
colours; opacity 1, background 1), the reference is the oracle alone
(oracle.render_sum, and its backward chained through the projection VJP), and
nothing of gsvc_amd is imported.

A sequence is a list of Steps (model, H, W); a Model that appears twice is the
same object, so "the same inputs earlier in the sequence" is an identity test.
References are computed once per (model, H, W) and shared, never modified.

Splat counts: test_torch_ops.py's order test needs n = 7777 to be a count no
other test uses (its first call must start without an order).  Every count
here is one of COUNTS; keep 7777 out of it.
"""
import functools

import numpy as np

import oracle as O

F32 = np.float32
COUNTS = (0, 1, 150, 300, 1400, 1500, 1700, 3000)
assert 7777 not in COUNTS
BORDERLINE = 1e-5          # test_gpu_parity._check_final_idx's definition
BANDED_PER_TILE = 96       # raster_sum.hip kDenseEntriesPerTile: M hint > 96 * tiles -> banded
NARROW, WIDE = 256, 1024   # entries per tile: blended / held by the wide id slab
OFFSCREEN = 50.0           # added to means2d: no tile intersects (test_cpp_function_planar_output)
BASE = 64                  # base image side: 16 tiles


def borderline_cap(H, W):
    """0.1 % of the pixels, rounded down: 4 for 64 x 64."""
    return H * W // 1024


def ntiles(H, W):
    return ((H + 15) // 16) * ((W + 15) // 16)


class Model:
    """One frame model; ``kind`` names the density class it must have at
    64 x 64 (None: no claim)."""

    def __init__(self, name, means, L, colors, kind=None):
        assert len(means) in COUNTS, len(means)
        self.name, self.kind = name, kind
        self.means = np.ascontiguousarray(means, F32)
        self.L = np.ascontiguousarray(L, F32)
        self.colors = np.ascontiguousarray(colors, F32)
        for a in (self.means, self.L, self.colors):
            a.setflags(write=False)

    @property
    def n(self):
        return len(self.means)


class Step:
    def __init__(self, model, H=BASE, W=BASE):
        self.model, self.H, self.W = model, H, W

    @property
    def key(self):
        return (id(self.model), self.H, self.W)


class Ref:
    """The oracle's frame: out [H, W, 3] (unclamped, the op path's image),
    planes [3, H, W] (clamped, the render paths'), ok [H, W] (False on
    borderline pixels), M, the densest tile's entry count."""

    def __init__(self, step):
        m, H, W = step.model, step.H, step.W
        self.H, self.W, self.n = H, W, m.n
        opac = np.ones((m.n, 1), F32)
        if m.n == 0:
            r = dict(out=np.ones((H, W, 3), F32), m=0)
        else:
            r = O.render_sum(m.means, m.L, m.colors, opac, H, W)
        self.r = r
        self.m = int(r["m"])
        self.out = r["out"]
        self.planes = np.ascontiguousarray(np.clip(r["out"], 0, 1).transpose(2, 0, 1))
        nt = ntiles(H, W)
        if self.m > 0:
            margin = O.sum_min_margin(r["tb"], H, W, r["gids_sorted"], r["bins"], r["xys"],
                                      r["conics"], opac)
            self.ok = ~(margin < BORDERLINE)
            bins = np.asarray(r["bins"])[:nt]
            self.tile_max = int((bins[:, 1] - bins[:, 0]).max())
        else:
            self.ok = np.ones((H, W), bool)
            self.tile_max = 0
        self.borderline = int((~self.ok).sum())
        self._grads = None
        self._model = m

    def grads(self):
        """(v_means2d, v_L, v_colors) for v_out(H, W): raster_sum_backward on
        the oracle's own final_idx, then project_2d_backward."""
        if self._grads is None:
            m, r = self._model, self.r
            if self.m < 1:
                self._grads = (np.zeros((m.n, 2), F32), np.zeros((m.n, 3), F32),
                               np.zeros((m.n, 3), F32))
            else:
                opac = np.ones((m.n, 1), F32)
                v_xy, v_conic, v_rgb, _ = O.raster_sum_backward(
                    r["tb"], self.H, self.W, r["gids_sorted"], r["bins"], r["xys"], r["conics"],
                    m.colors, opac, r["final_idx"], v_out(self.H, self.W))
                _, v_mean, v_L = O.project_2d_backward(m.L, self.H, self.W, r["radii"], r["conics"],
                                                       v_xy.astype(F32), v_conic.astype(F32))
                self._grads = (v_mean, v_L, v_rgb)
        return self._grads


_refs = {}


def ref(step):
    """The shared reference of a step (one oracle call per distinct frame)."""
    got = _refs.get(step.key)
    if got is None or got[0] is not step.model:
        got = _refs[step.key] = (step.model, Ref(step))
    return got[1]


@functools.lru_cache(maxsize=None)
def v_out(H, W):
    """The upstream gradient of the op path's backward, fixed per shape."""
    v = np.random.default_rng(1000 * H + W).standard_normal((H, W, 3)).astype(F32)
    v.setflags(write=False)
    return v


# ---------------------------------------------------------------- models

def frame(n, seed, chol_scale=1.0, kind=None, name=None):
    means, L, colors, _ = O.synthetic_frame(n, seed, chol_scale=chol_scale)
    return Model(name or f"n{n}_s{seed}_c{chol_scale:g}", means, L, colors, kind)


def shifted(m, kind="empty"):
    return Model(m.name + "_off", m.means + F32(OFFSCREEN), m.L, m.colors, kind)


def scaled(m, factor, kind):
    return Model(f"{m.name}_x{factor:g}", m.means, m.L * F32(factor), m.colors, kind)


def mostly_off(m, seed, share=0.9, kind="sparse"):
    """``share`` of the splats moved off-screen: the same N, a sparse frame."""
    off = np.random.default_rng(seed).random(m.n) < share
    means = m.means.copy()
    means[off] += F32(OFFSCREEN)
    return Model(f"{m.name}_sp{seed}", means, m.L, m.colors, kind)


def head(m, n):
    return Model(f"{m.name}_h{n}", m.means[:n], m.L[:n], m.colors[:n])


def joined(a, b):
    return Model(f"{a.name}+{b.name}", np.concatenate([a.means, b.means]),
                 np.concatenate([a.L, b.L]), np.concatenate([a.colors, b.colors]))


# ---------------------------------------------------------------- sequences
# Seeds: chosen so that every frame passes test_premises (a seed that does not
# is replaced, not excused).

PHASE = 34  # calls per phase: two of the 16-call hint copies land in each


@functools.lru_cache(maxsize=None)
def alternation():
    """1: two dense256 models of equal N; 66 calls A, B, ... then 66 calls
    B, A, ...: refreshes 64 calls apart fall on index r and r + 64 (r + 128),
    which the swap at 66 gives to different models whatever r is."""
    a = frame(3000, 0, kind="dense256")
    b = frame(3000, 1, kind="dense256")
    return [Step((a, b)[(i + (i >= 66)) % 2]) for i in range(132)]


@functools.lru_cache(maxsize=None)
def drift():
    """2: n = 1500, 70 positions of a random walk (0.05 NDC per call), L scaled
    by 1.1 + 0.4 sin: a tenth starts off-screen and walks in, a tenth walks
    out; a last step repeats step 0's model."""
    n, calls = 1500, 70
    base = frame(n, 2)
    rng = np.random.default_rng(12)
    means = base.means.copy()
    inward, outward = slice(0, n // 10), slice(n // 10, n // 5)
    means[inward, 0] = F32(1.6) + F32(0.4) * rng.random(n // 10, dtype=F32)
    bias = np.zeros((n, 2), F32)
    bias[inward, 0] = -0.03
    bias[outward, 0] = 0.03
    steps = []
    for k in range(calls):
        s = F32(1.1 + 0.4 * np.sin(2 * np.pi * k / calls))
        steps.append(Step(Model(f"drift{k}", means, base.L * s, base.colors)))
        ang = rng.random(n) * 2 * np.pi
        means = (means + F32(0.05) * np.stack([np.cos(ang), np.sin(ang)], 1).astype(F32)
                 + bias).astype(F32)
    steps.append(Step(steps[0].model))
    return steps


@functools.lru_cache(maxsize=None)
def swings_same_n():
    """3: one 3000-splat model; only the means and the L scale change."""
    d256 = frame(3000, 3, kind="dense256")
    sp = mostly_off(d256, 5)
    phases = [sp, scaled(d256, 3.0, "dense1024"), shifted(d256), d256, sp]
    return [[Step(m)] * PHASE for m in phases]


@functools.lru_cache(maxsize=None)
def swings_changing_n():
    """4: the same classes with N changing between phases."""
    sp = frame(300, 4, kind="sparse")
    phases = [sp, frame(3000, 5, 3.0, kind="dense1024"), shifted(frame(1500, 2)),
              frame(3000, 0, kind="dense256"), sp]
    return [[Step(m)] * PHASE for m in phases]


@functools.lru_cache(maxsize=None)
def shapes():
    """5: prune, densify, two 28-tile shapes of different tbx, one splat, a
    ragged shape, and back; three calls per step."""
    a = frame(1500, 2)
    pruned = head(a, 1400)
    dens = joined(pruned, frame(300, 4))
    one = head(frame(300, 4), 1)
    plan = [(a, 64, 64), (pruned, 64, 64), (dens, 64, 64), (dens, 60, 100), (dens, 100, 60),
            (dens, 64, 64), (one, 64, 64), (a, 37, 53), (a, 64, 64)]
    return [[Step(m, H, W)] * 3 for m, H, W in plan]


@functools.lru_cache(maxsize=None)
def backward_pair():
    """6: two models of equal N for backwards that follow other forwards."""
    return Step(frame(1500, 2)), Step(frame(1500, 6))


@functools.lru_cache(maxsize=None)
def two_streams():
    """7: dense1024 on one stream, sparse on the other."""
    return Step(frame(3000, 5, 3.0, kind="dense1024")), Step(frame(300, 4, kind="sparse"))


@functools.lru_cache(maxsize=None)
def no_splats():
    """9: a frame with intersections, a model of no splats, then a model whose
    splats are all off-screen (M = 0 with N > 0), and the first again; twice,
    three calls apart, so each meets both parities."""
    x = frame(300, 4, kind="sparse")
    none = Model("none", np.zeros((0, 2), F32), np.zeros((0, 3), F32), np.zeros((0, 3), F32),
                 "empty")
    off = shifted(frame(300, 7))
    return [Step(m) for m in (x, none, off, x, none, off, x)]


GOP_CALLS = 18  # per list: the 16-call hint copy turns over in each


@functools.lru_cache(maxsize=None)
def gop_lists():
    """8: F = 4 at 64 x 64.  Each entry: (models of the four frames, calls,
    class of the whole list by its summed M against 96 * tiles * F)."""
    sp = [frame(300, s, kind="sparse") for s in (4, 7, 8, 9)]
    d1024 = [frame(3000, s, 3.0, kind="dense1024") for s in (5, 10, 11, 12)]
    none = Model("none", np.zeros((0, 2), F32), np.zeros((0, 3), F32), np.zeros((0, 3), F32),
                 "empty")
    one = head(sp[1], 1)
    return [
        (sp, GOP_CALLS, "sparse"),
        ([d1024[0], one, none, sp[3]], GOP_CALLS, "dense"),
        ([none] * 4, GOP_CALLS, "empty"),
        (d1024, GOP_CALLS, "dense"),
        (sp, GOP_CALLS, "sparse"),
        # total N shrinking and growing under the same (F, H, W)
        ([head(sp[0], 150), sp[1], none, sp[3]], 3, "sparse"),
        ([sp[0], sp[1], d1024[2], sp[3]], 3, "dense"),
        (sp, 3, "sparse"),
    ]


def all_steps():
    """name -> every step of the sequence (the premise tests walk these)."""
    flat = lambda phases: [s for p in phases for s in p]  # noqa: E731
    return {
        "alternation": alternation(),
        "drift": drift(),
        "swings_same_n": flat(swings_same_n()),
        "swings_changing_n": flat(swings_changing_n()),
        "shapes": flat(shapes()),
        "backward_pair": list(backward_pair()),
        "two_streams": list(two_streams()),
        "no_splats": no_splats(),
        "gop": [Step(m) for models, _, _ in gop_lists() for m in models],
    }


def distinct(steps):
    seen, out = set(), []
    for s in steps:
        if s.key not in seen:
            seen.add(s.key)
            out.append(s)
    return out


def check_class(kind, r):
    """The density class ``kind`` as the kernels' thresholds see it."""
    dense = BANDED_PER_TILE * ntiles(r.H, r.W)
    if kind == "empty":
        assert r.m == 0
    elif kind == "sparse":
        assert 0 < r.m < dense and r.tile_max <= NARROW, (r.m, r.tile_max)
    elif kind == "dense256":
        assert r.m > dense and NARROW < r.tile_max <= WIDE, (r.m, r.tile_max)
    elif kind == "dense1024":
        assert r.m > dense and r.tile_max > WIDE, (r.m, r.tile_max)
    else:
        assert kind is None, kind
