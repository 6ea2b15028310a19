"""GPU: the filtered composite (csrc/resample_aa.hip) -- bit for bit against the
two-pass statement of its rule (the fine view's image from the point-sampled
composite, reduced by cpu.box_reduce_view) on views whose seams are asserted
first, against the native render at integer downscales, with poisoned seam
parts, against the CPU statement, and through decode_frames / decode_video /
the command line."""
import ctypes

import numpy as np
import pytest
import torch

import resample_aa_cases as AC
import resample_cases as RC
from gsvc_amd import codec
from gsvc_amd import compress as C
from gsvc_amd.cpu import box_reduce_view
from gsvc_amd.render import View, render_frames_sum
from gsvc_amd.video import YuvFormat, rgb_to_i420

pytestmark = pytest.mark.gpu


def _view(name, size, crop, aa):
    c = RC.case(name)
    return c, View(c["H"], c["W"], size=size, crop=crop, aa=aa)


@pytest.fixture(scope="module")
def two_pass(cuda):
    """box_reduce_view of the fine view's GPU image, per FUSED row, computed once."""
    cache = {}

    def get(i):
        if i not in cache:
            name, size, crop, aa = AC.FUSED[i][:4]
            c, view = _view(name, size, crop, aa)
            cache[i] = box_reduce_view(RC.render(c, cuda, view.fine).cpu(), view)
        return cache[i]
    return get


@pytest.mark.parametrize("name", RC.CASES)
def test_aa_of_one_is_the_point_sampled_view(cuda, name):
    c = RC.case(name)
    kw = dict(size=(c["H"] // 2 + 1, c["W"] // 3))
    want = RC.render(c, cuda, View(c["H"], c["W"], **kw))
    assert torch.equal(RC.render(c, cuda, View(c["H"], c["W"], aa=(1, 1), **kw)), want)
    assert torch.equal(RC.render(c, cuda, View(c["H"], c["W"], aa=1, **kw)), want)


@pytest.mark.parametrize("i", range(len(AC.FUSED)), ids=AC.FUSED_IDS)
def test_fused_is_the_two_pass_result(cuda, i, two_pass):
    name, size, crop, aa, seam_rows, seam_cols = AC.FUSED[i]
    c, view = _view(name, size, crop, aa)
    assert AC.seams(view) == (seam_rows, seam_cols)
    got = RC.render(c, cuda, view)
    assert got.shape == (len(c["sizes"]), 3) + tuple(size)
    want = two_pass(i)
    diff = float((got.cpu() - want).abs().max())
    print(f"{AC.FUSED_IDS[i]}: seams {AC.seams(view)}, max |fused - two-pass| = {diff:.3e}")
    assert torch.equal(got.cpu(), want)
    if name == "batch":  # the M = 0 frame: the clamped background, n equal values summed and divided
        bg = torch.tensor([0.25, 1.0, 0.0]).view(3, 1, 1)
        assert float((got[1].cpu() - bg).abs().max()) <= aa[0] * aa[1] * 2.0 ** -24


@pytest.mark.parametrize("name,k", [("piled", 4), ("wide", 4), ("wide", 8)])
def test_integer_downscale_is_the_reduced_native_render(cuda, name, k):
    c = RC.case(name)
    view = View(c["H"], c["W"], size=(c["H"] // k, c["W"] // k), aa=k)
    assert view.fine.is_identity
    native = RC.render(c, cuda)
    assert torch.equal(RC.render(c, cuda, view).cpu(), box_reduce_view(native.cpu(), view))


def _entry_call(cuda, c, view, parts, bufs, call_index, **kw):
    """gsvc_render_frames_filtered through _lib on the case's tensors; ``bufs``
    holds the workspace, meta and offsets between calls."""
    from gsvc_amd import _lib as L
    lib = L.load()
    F, n, H, W = len(c["sizes"]), int(c["means"].shape[0]), c["H"], c["W"]
    if not bufs:
        t = lambda x: x.to(cuda).contiguous()
        bufs.update(means=t(c["means"]), chol=t(c["chol"]), col=t(c["col"]), bg=t(c["bg"]),
                    bound=t(torch.tensor(RC.BOUND)))
        need = L.size("gsvc_render_frames_workspace_bytes", F, n, H, W)
        bufs["ws"] = torch.empty((need,), dtype=torch.uint8, device=cuda)
        bufs["ws"][: L.size("gsvc_render_frames_zeroed_bytes", F, H, W)].zero_()
        bufs["meta"] = torch.zeros((F, 2), dtype=torch.int32, device=cuda)
        offs = [0]
        for x in c["sizes"]:
            offs.append(offs[-1] + x)
        bufs["offs_host"] = (ctypes.c_int * (F + 1))(*offs)
        bufs["offs"] = torch.tensor(offs, dtype=torch.int32, device=cuda)
    host = [a.copy() for a in view.fine.host_tables()]
    for key, idx in (("sx", 0), ("sy", 1), ("cs", 2), ("rs", 3)):
        if key in kw:
            host[idx] = kw[key]
    tabs = [torch.from_numpy(a).to(cuda) for a in host]
    out = torch.full((F, 3, view.out_h, view.out_w), -7.0, dtype=torch.float32, device=cuda)
    ky, kx = kw.get("aa", view.aa)
    parts_ptr = 0 if parts is None else parts.data_ptr()
    parts_bytes = kw.get("parts_bytes", 0 if parts is None else 4 * parts.numel())
    stream = torch.cuda.current_stream(cuda).cuda_stream
    rc = lib.gsvc_render_frames_filtered(
        F, bufs["offs_host"], bufs["offs"].data_ptr(), bufs["means"].data_ptr(), 0, bufs["chol"].data_ptr(),
        bufs["bound"].data_ptr(), bufs["col"].data_ptr(), None, None, bufs["bg"].data_ptr(), H, W, call_index,
        0, bufs["meta"].data_ptr(), bufs["ws"].data_ptr(), bufs["ws"].numel(), host[0].ctypes.data,
        host[1].ctypes.data, host[2].ctypes.data, host[3].ctypes.data, tabs[0].data_ptr(), tabs[1].data_ptr(),
        tabs[2].data_ptr(), tabs[3].data_ptr(), ky, kx, kw.get("out_h", view.out_h),
        kw.get("out_w", view.out_w), parts_ptr, parts_bytes, out.data_ptr(), stream)
    torch.cuda.synchronize(cuda)
    return rc, out, lib.gsvc_last_error()


@pytest.mark.parametrize("i", [0, 5], ids=[AC.FUSED_IDS[0], AC.FUSED_IDS[5]])
def test_seam_parts_are_written_before_they_are_read(cuda, i, two_pass):
    """Poisoned parts change nothing: every slot the second kernel reads was
    written by this call."""
    name, size, crop, aa = AC.FUSED[i][:4]
    c, view = _view(name, size, crop, aa)
    count = 12 * len(c["sizes"]) * size[0] * size[1]
    bufs, outs = {}, []
    for call, poison in enumerate((float("nan"), 1e30)):
        parts = torch.full((count,), poison, dtype=torch.float32, device=cuda)
        rc, out, msg = _entry_call(cuda, c, view, parts, bufs, call)
        assert rc == 0, msg
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], two_pass(i))


def test_entries_alternate_on_one_workspace(cuda, two_pass):
    c, view = _view(*AC.FUSED[0][:4])
    native = RC.render(c, cuda)
    point = RC.render(c, cuda, View(c["H"], c["W"], size=(12, 17)))
    for _ in range(2):
        assert torch.equal(RC.render(c, cuda, view).cpu(), two_pass(0))
        assert torch.equal(RC.render(c, cuda, view).cpu(), two_pass(0))  # two consecutive calls
        assert torch.equal(RC.render(c, cuda), native)
        assert torch.equal(RC.render(c, cuda, View(c["H"], c["W"], size=(12, 17))), point)


@pytest.mark.parametrize("name", RC.CASES)
@pytest.mark.parametrize("which", ["half", "quarter-auto"])
def test_against_the_cpu_statement(cuda, name, which):
    c = RC.case(name)
    H, W = c["H"], c["W"]
    view = (View(H, W, size=(H // 2, W // 2), aa=2) if which == "half"
            else View(H, W, size=(H // 4, W // 4), aa="auto"))
    got = RC.render(c, cuda, view).cpu().numpy()
    want = RC.render(c, "cpu", view).numpy()
    print(f"{name} {which}: aa {view.aa}, max |gpu - cpu| = {float(np.max(np.abs(got - want))):.3e}")
    np.testing.assert_allclose(got, want, rtol=RC.IMG_RTOL, atol=RC.IMG_ATOL)


# --------------------------------------------------------------------------
# decode_frames / decode_video / the command line

@pytest.mark.parametrize("kw", [dict(size=(24, 40), aa=2), dict(size=(9, 13), crop=(10.25, 3.5, 60.5, 40.0), aa=(4, 4)),
                                dict(aa=(2, 3))])
def test_decode_frames_aa(cuda, kw):
    streams = RC.stream()
    view = View(RC.STREAM_H, RC.STREAM_W, **kw)
    imgs, state = C.decode_frames(streams, cuda, return_state=True, **kw)
    xq, Lq, cq, _, sizes, (H, W) = C.unpack_frames(streams, cuda)
    want = render_frames_sum(xq, Lq, cq, sizes, H, W, torch.ones(3, device=cuda), view=view)
    assert imgs.shape == (3, 3, view.out_h, view.out_w) and torch.equal(imgs, want)
    _, state0 = C.decode_frames(streams, cuda, return_state=True)
    assert all(torch.equal(a, b) for a, b in zip(state, state0))


@pytest.mark.parametrize("fmt", [None, YuvFormat.from_pix_fmt("yuv420p10le"), YuvFormat.from_pix_fmt("nv12")])
def test_decode_frames_i420_aa(cuda, fmt):
    streams = RC.stream()
    kw = dict(size=(24, 40), aa=2)
    imgs = C.decode_frames(streams, cuda, **kw)
    yuv = C.decode_frames(streams, cuda, output="i420", fmt=fmt, **kw)
    assert yuv.shape == (3, (fmt or YuvFormat()).frame_bytes(24, 40))
    assert torch.equal(yuv, rgb_to_i420(imgs, None, fmt))


def test_decode_video_and_command_line_aa(cuda, tmp_path):
    streams = RC.stream()
    fmt = YuvFormat()
    outs = []
    for batch in (1, 8):
        path = tmp_path / f"b{batch}.yuv"
        res = codec.decode_video(streams, path, device=cuda, batch=batch, size=(24, 40), aa=2)
        assert res["bytes_written"] == 3 * fmt.frame_bytes(24, 40) and (res["height"], res["width"]) == (24, 40)
        outs.append(path.read_bytes())
    assert outs[0] == outs[1]
    assert outs[0] == C.decode_frames(streams, cuda, output="i420", size=(24, 40), aa=2).cpu().numpy().tobytes()
    assert outs[0] != C.decode_frames(streams, cuda, output="i420", size=(24, 40)).cpu().numpy().tobytes()
    codec.write_video(tmp_path / "v.gsvf", streams)
    for aa in ("2", "auto", "2x2"):  # 48 x 80 -> 24 x 40: auto is 2 x 2
        codec.main(["decode", str(tmp_path / "v.gsvf"), str(tmp_path / f"cli_{aa}.yuv"), "--device", str(cuda),
                    "--size", "40x24", "--aa", aa])
        assert (tmp_path / f"cli_{aa}.yuv").read_bytes() == outs[0], aa


# --------------------------------------------------------------------------
# the entry's checks

def test_entry_refuses_bad_arguments_before_any_launch(cuda):
    """GSVC_ERR_ARG (1) for ky kx = 72, a null or short ``parts``, tables that
    do not partition the fine size and tables that put a pixel on three tiles;
    nothing is launched: ``out`` keeps its fill and the next call on the
    workspace is right."""
    c, view = _view(*AC.FUSED[0][:4])
    count = 12 * 12 * 17
    parts = torch.empty((count,), dtype=torch.float32, device=cuda)
    bufs = {}
    sx, sy, cs, rs = (a.copy() for a in view.fine.host_tables())

    def refused(word, parts_=parts, **kw):
        rc, out, msg = _entry_call(cuda, c, view, parts_, bufs, 0, **kw)
        assert rc == 1 and word in msg, (kw, rc, msg)
        assert bool((out == -7.0).all())

    refused(b"ky kx", aa=(9, 8))
    refused(b"ky kx", aa=(0, 3))
    refused(b"missing", parts_=None)
    refused(b"parts", parts_bytes=4 * count - 4)
    bad = cs.copy()
    bad[1] += 1
    bad[2] = bad[1] - 1
    refused(b"partition", cs=bad)
    refused(b"partition", out_h=11)  # the fine tables are of 36 rows, not 33
    # rows: all of tile 1's samples given to tiles 0 and 2 -> pixels whose rows lie on tiles 0, (1,) 2
    three = rs.copy()
    cut = int(rs[1] + rs[2]) // 2
    cut += cut % 3 == 0  # the cut falls inside a pixel
    three[1] = three[2] = cut
    refused(b"more than two tiles", rs=three)
    rc, out, msg = _entry_call(cuda, c, view, parts, bufs, 0)
    assert rc == 0 and torch.equal(out, RC.render(c, cuda, view))
