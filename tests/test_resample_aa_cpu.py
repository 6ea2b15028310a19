"""CPU: views with ``aa`` (the box prefilter of include/gsvc_amd.h
gsvc_render_frames_filtered) -- validation, the equivalences with plain views,
the <= 2 tiles rule against its restatement, ``cpu.box_reduce_view`` against a
float64 mean and against the native render where the relation is exact,
``decode_frames(aa=)``, and that the filter reduces aliasing."""
import numpy as np
import pytest
import torch

import resample_aa_cases as AC
import resample_cases as RC
from gsvc_amd import compress as C
from gsvc_amd.cpu import box_reduce_view
from gsvc_amd.render import View, render_frames_sum, view_of


@pytest.mark.parametrize("aa", [0, (9, 8), 2.5, -1, (2, 0), (2, 2, 2), "automatic", (65, 1)])
def test_bad_aa(aa):
    with pytest.raises(ValueError):
        View(64, 64, size=(16, 16), aa=aa)


def test_more_than_two_tiles_is_an_error():
    with pytest.raises(ValueError):
        View(64, 64, size=(1, 1), aa=8)  # sub-samples at 3.5, 11.5, ...: four tiles
    View(64, 64, size=(2, 2), aa=8)  # two tiles per pixel
    with pytest.raises(ValueError):
        view_of(64, 64, size=(1, 1), aa=8)
    with pytest.raises(ValueError):
        C.decode_frames(RC.stream(), "cpu", size=(1, 1), aa=(8, 1))  # 48 rows: three tiles


def _same_tables(a, b):
    return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a.host_tables(), b.host_tables()))


@pytest.mark.parametrize("aa", [None, 1, (1, 1)])
def test_aa_of_one_is_the_plain_view(aa):
    c = RC.case("edge")
    kw = dict(size=(20, 31), crop=(3.5, 2.25, 40.0, 30.5))
    plain, v = View(c["H"], c["W"], **kw), View(c["H"], c["W"], aa=aa, **kw)
    assert v.aa == (1, 1) and v.fine is v and _same_tables(v, plain)
    assert torch.equal(RC.render(c, "cpu", v), RC.render(c, "cpu", plain))


@pytest.mark.parametrize("kw", [dict(size=(12, 17), aa=(3, 3)), dict(size=(9, 20), aa=(4, 1)),
                                dict(size=(6, 10), crop=(10.25, 3.5, 30.5, 24.0), aa=(2, 5)), dict(aa=2)])
def test_fine_view(kw):
    v = View(37, 53, **kw)
    ky, kx = v.aa
    fine = View(37, 53, (ky * v.out_h, kx * v.out_w), kw.get("crop"))
    assert (v.fine.out_h, v.fine.out_w) == (ky * v.out_h, kx * v.out_w) and v.fine.aa == (1, 1)
    assert _same_tables(v.fine, fine)
    # the view's own tables stay those of the point-sampled view of its size
    assert _same_tables(v, View(37, 53, kw.get("size"), kw.get("crop")))
    assert view_of(37, 53, aa=v.aa, **{k: kw[k] for k in kw if k != "aa"}) is \
        view_of(37, 53, aa=v.aa, **{k: kw[k] for k in kw if k != "aa"})
    assert view_of(37, 53, kw.get("size"), kw.get("crop"), aa=v.aa).aa == v.aa
    assert view_of(37, 53, kw.get("size"), kw.get("crop")).aa == (1, 1)


def test_auto():
    assert View(1080, 1920, size=(270, 480), aa="auto").aa == (4, 4)
    assert View(1080, 1920, size=(540, 960), aa="auto").aa == (2, 2)
    assert View(1080, 1920, size=(2160, 3840), aa="auto").aa == (1, 1)  # an upscale
    assert View(1080, 1920, size=(500, 1920), aa="auto").aa == (3, 1)  # ceil, per axis
    assert View(1080, 1920, size=(135, 240), crop=(0, 0, 960, 540), aa="auto").aa == (4, 4)  # the window's extent
    assert View(1080, 1920, size=(108, 192), aa="auto").aa == (8, 8)  # at most 8


def test_two_tiles_rule_against_its_restatement():
    """View raises exactly where the rule's text says so, over source sizes
    1..70, output sizes 1..40 and k in {1, 2, 3, 4, 5, 8}, the whole axis and a
    fractional window of it (columns carry the axis under test; rows are a
    single tile, which never fails)."""
    checked = refused = 0
    for src in range(1, 71):
        windows = [(0.0, float(src))]
        if src >= 3:
            windows.append((0.75, src - 1.5))
        for out in range(1, 41):
            for k in (1, 2, 3, 4, 5, 8):
                for x0, w in windows:
                    want = AC.two_tiles_ok(src, out, x0, w, k)
                    try:
                        View(8, src, size=(1, out), crop=(x0, 0, w, 8), aa=(1, k))
                        got = True
                    except ValueError:
                        got = False
                    assert got == want, (src, out, k, x0, w, got, want)
                    checked += 1
                    refused += not want
    print(f"{checked} views, {refused} refused")
    assert refused > 0 and refused < checked


@pytest.mark.parametrize("name,size,crop,aa", [f[:4] for f in AC.FUSED], ids=AC.FUSED_IDS)
def test_box_reduce_against_a_float64_mean(name, size, crop, aa):
    """|box_reduce_view - float64 block mean| <= ky kx 2^-24: n values in [0, 1]
    summed in any order carry at most (n - 1) 2^-24 relative to n, and the
    division adds at most half an ulp of a value <= 1."""
    c = RC.case(name)
    view = View(c["H"], c["W"], size=size, crop=crop, aa=aa)
    gen = torch.Generator().manual_seed(5)
    fine = torch.rand(2, 3, aa[0] * size[0], aa[1] * size[1], generator=gen)
    fine[0, 0, :aa[0]] = 1.0  # a saturated row of pixels
    got = box_reduce_view(fine, view)
    assert got.dtype == torch.float32 and got.shape == (2, 3) + tuple(size)
    want = fine.double().reshape(2, 3, size[0], aa[0], size[1], aa[1]).mean(dim=(3, 5))
    err = float((got.double() - want).abs().max())
    print(f"{name} {size} aa {aa}: max |float32 rule - float64 mean| = {err:.3e}")
    assert err <= aa[0] * aa[1] * 2.0 ** -24
    assert np.array_equal(box_reduce_view(fine.numpy(), view), got.numpy())  # numpy in, numpy out


def _row_major_mean(img, ky, kx):
    """The plain row-major float32 sum over (a, b) from +0.0, divided."""
    acc = np.zeros(img.shape[:-2] + (img.shape[-2] // ky, img.shape[-1] // kx), dtype=np.float32)
    for a in range(ky):
        for b in range(kx):
            acc = acc + img[..., a::ky, b::kx]
    return acc / np.float32(ky * kx)


def _unpacked(streams):
    """The decoded parameters of every frame, concatenated, and their sizes."""
    frames = C.unpack_frames_host(streams)
    T = torch.from_numpy
    return (torch.cat([T(f[0]) for f in frames]), torch.cat([T(f[1]) for f in frames]),
            torch.cat([T(f[2]) for f in frames]), [f[0].shape[0] for f in frames])


@pytest.fixture(scope="module")
def stream_native():
    H, W = RC.STREAM_H, RC.STREAM_W
    args = _unpacked(RC.stream()) + (H, W, torch.ones(3))
    return args, C.decode_frames(RC.stream(), "cpu")  # the native render: the CPU operators


@pytest.mark.parametrize("k", [2, 4, 8])
def test_integer_downscale_of_the_stream_is_the_reduced_native_render(k, stream_native):
    """Sides that are multiples of k: the fine view of size=(H / k, W / k),
    aa=k is the identity view, so the result is box_reduce_view(native render)
    bit for bit -- and, where no pixel straddles a tile (k divides 16), the
    plain row-major sum."""
    args, native = stream_native
    H, W = RC.STREAM_H, RC.STREAM_W
    view = View(H, W, size=(H // k, W // k), aa=k)
    assert view.fine.is_identity and AC.seams(view) == (0, 0)
    got = render_frames_sum(*args, view=view)
    assert got.shape == (3, 3, H // k, W // k)
    assert torch.equal(got, box_reduce_view(native, view))
    assert np.array_equal(got.numpy(), _row_major_mean(native.numpy(), k, k))


def test_integer_downscale_of_piled():
    c = RC.case("piled")
    view = View(64, 64, size=(16, 16), aa=4)
    assert view.fine.is_identity
    native = RC.native_cpu(c)
    got = RC.render(c, "cpu", view)
    assert torch.equal(got, box_reduce_view(native, view))
    assert np.array_equal(got.numpy(), _row_major_mean(native.numpy(), 4, 4))


def test_slots_split_the_sum_at_a_seam():
    """A pixel that straddles a tile edge is NOT the plain row-major sum: each
    tile's part is summed on its own, then the parts are added in slot order."""
    view = View(37, 53, size=(12, 17), aa=3)
    assert AC.seams(view) == (2, 2)
    fine = torch.rand(3, 36, 51, generator=torch.Generator().manual_seed(9))
    got = box_reduce_view(fine, view).numpy()
    f = fine.numpy()
    tr, tc = (view.fine.py >> 4).reshape(12, 3), (view.fine.px >> 4).reshape(17, 3)
    for i in range(12):
        for j in range(17):
            parts = {}
            for a in range(3):
                for b in range(3):
                    slot = 2 * int(tr[i, a] - tr[i, 0]) + int(tc[j, b] - tc[j, 0])
                    parts[slot] = parts.get(slot, np.zeros(3, np.float32)) + f[:, 3 * i + a, 3 * j + b]
            total = None
            for slot in sorted(parts):
                total = parts[slot] if total is None else total + parts[slot]
            assert np.array_equal(got[:, i, j], total / np.float32(9)), (i, j)
    corner = [(i, j) for i in range(12) for j in range(17) if tr[i, 0] != tr[i, 2] and tc[j, 0] != tc[j, 2]]
    assert len(corner) == 4


@pytest.mark.parametrize("kw", [dict(size=(24, 40), aa=2), dict(size=(12, 20), aa="auto"), dict(aa=(2, 3)),
                                dict(size=(9, 13), crop=(10.25, 3.5, 60.5, 40.0), aa=(4, 4))])
def test_decode_frames_aa_cpu(kw):
    streams = RC.stream()
    view = View(RC.STREAM_H, RC.STREAM_W, **kw)
    imgs, state = C.decode_frames(streams, "cpu", return_state=True, **kw)
    xq, Lq, cq, sizes = _unpacked(streams)
    H, W = RC.STREAM_H, RC.STREAM_W
    want = render_frames_sum(xq, Lq, cq, sizes, H, W, torch.ones(3), view=view)
    assert imgs.shape == (3, 3, view.out_h, view.out_w) and torch.equal(imgs, want)
    assert torch.equal(want, box_reduce_view(render_frames_sum(xq, Lq, cq, sizes, H, W, torch.ones(3),
                                                               view=view.fine), view))
    _, state0 = C.decode_frames(streams, "cpu", return_state=True)
    assert all(torch.equal(a, b) for a, b in zip(state, state0))


def test_entry_refuses_bad_arguments_without_a_device():
    """gsvc_render_frames_filtered returns GSVC_ERR_ARG from its host checks
    before any launch: this runs without a device, and the stand-in device
    pointers are never dereferenced."""
    import ctypes
    from gsvc_amd import _lib
    lib = _lib.load_product()
    H, W = 37, 53
    v = View(H, W, size=(12, 17), aa=3)
    sx, sy, cs, rs = (a.copy() for a in v.fine.host_tables())
    offs = (ctypes.c_int * 2)(0, 5)
    fake = 0x1000
    need = 4 * 12 * 12 * 17

    def call(ky=3, kx=3, out_h=12, out_w=17, parts=fake, parts_bytes=need, cs=cs, rs=rs):
        rc = lib.gsvc_render_frames_filtered(
            1, offs, fake, fake, 0, fake, None, fake, None, None, fake, H, W, 0, 0, fake, fake, 1 << 30,
            sx.ctypes.data, sy.ctypes.data, cs.ctypes.data, rs.ctypes.data, fake, fake, fake, fake, ky, kx,
            out_h, out_w, parts, parts_bytes, fake, None)
        return rc, lib.gsvc_last_error()

    for kw, word in ((dict(ky=9, kx=8), b"ky kx"), (dict(ky=0), b"ky kx"), (dict(kx=65, ky=1), b"ky kx"),
                     (dict(parts=None), b"missing"), (dict(parts_bytes=need - 1), b"parts"),
                     (dict(parts_bytes=0), b"parts"), (dict(out_h=11), b"partition"),
                     (dict(out_w=18), b"partition"), (dict(out_h=0), b"bad sizes")):
        rc, msg = call(**kw)
        assert rc == 1 and word in msg, (kw, rc, msg)
    cut = int(rs[1] + rs[2]) // 2
    cut += cut % 3 == 0  # inside a pixel: its rows lie on tiles 0 and 2
    three = rs.copy()
    three[1] = three[2] = cut
    rc, msg = call(rs=three)
    assert rc == 1 and b"more than two tiles" in msg, (rc, msg)


def test_the_filter_reduces_aliasing():
    """Splats about 0.6 px wide seen through a 16 x 16 view of a 64 x 64 frame:
    against the float64 mean over every 4 x 4 block of source pixels of the
    frame at 8x supersampling (32 x 32 samples of the 512 x 512 view), the
    filtered view's mean absolute error is below the point-sampled view's."""
    c = AC.tiny_splats()
    H = W = 64
    truth = RC.render(c, "cpu", View(H, W, size=(512, 512)))[0].double()
    truth = truth.reshape(3, 16, 32, 16, 32).mean(dim=(2, 4))
    point = RC.render(c, "cpu", View(H, W, size=(16, 16)))[0].double()
    boxed = RC.render(c, "cpu", View(H, W, size=(16, 16), aa=4))[0].double()
    e_point, e_boxed = float((point - truth).abs().mean()), float((boxed - truth).abs().mean())
    print(f"mean |view - truth|: point-sampled {e_point:.5f}, aa=4 {e_boxed:.5f} (truth mean {float(truth.mean()):.5f})")
    assert float(truth.mean()) > 0.01  # the splats are seen at all
    assert e_boxed < e_point
