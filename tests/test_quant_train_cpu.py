"""CPU: the fused quantized training step's C entries are declared, bound and
refuse bad arguments before any launch; ``train_iter_quantize_fused`` raises
where it cannot run and changes nothing; and the float64 restatement of
``ResidualVQ8.ema_update`` (tests/quant_train_cases.py) agrees with the torch
one -- its fp32 error against the restatement is where the GPU test's bar for
``embed_avg`` and ``codebooks`` comes from."""
import ctypes
import os

import numpy as np
import pytest
import torch

import quant_cases as Q
import quant_train_cases as QT
from conftest import REPO

HEADER = os.path.join(REPO, "include", "gsvc_amd.h")


def test_symbols_and_abi():
    from gsvc_amd import _lib
    names = _lib.symbols()
    for n in ("gsvc_quant_train_workspace_bytes", "gsvc_quant_train_step", "gsvc_quant_adan_step"):
        assert n in names, n
    lib = _lib.load()
    assert lib.gsvc_abi_version() == _lib.ABI_VERSION == 4
    # xq, Lq, cq, the records [N,9] and the codes, plus the partials
    assert lib.gsvc_quant_train_workspace_bytes(1000) >= 1000 * (17 * 4 + 5)
    assert lib.gsvc_quant_train_workspace_bytes(1 << 20) > lib.gsvc_quant_train_workspace_bytes(1000)


def test_args_struct_layout(tmp_path):
    """compress._QuantStepArgs mirrors gsvc_quant_train_args field by field."""
    import shutil
    import subprocess
    from gsvc_amd.compress import _QuantStepArgs
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    names = [f[0] for f in _QuantStepArgs._fields_]
    body = "".join(f'printf("%zu ", offsetof(gsvc_quant_train_args, {n}));' for n in names)
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){%s'
                   'printf("%%zu\\n", sizeof(gsvc_quant_train_args));return 0;}\n' % (HEADER, body))
    exe = tmp_path / "off"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert got[:-1] == [getattr(_QuantStepArgs, n).offset for n in names]
    assert got[-1] == ctypes.sizeof(_QuantStepArgs)


def _dummy_args(n=10):
    """Arguments that pass every check up to the stream's: the pointers are
    never dereferenced, a failing check returns first."""
    from gsvc_amd import _lib
    lib = _lib.load()
    d = 16
    keep = dict(state=(ctypes.c_void_p * 20)(*([d] * 20)), hp=(ctypes.c_double * 10)(*QT.hparams(1)))
    a = QT.args_struct(
        n, xyz=d, cholesky=d, features=d, scale=d, beta=d, codebooks=d, cluster_size=d, embed_avg=d,
        cholesky_bound=d, background=d, gt=d, img_height=40, img_width=72, loss_kind=0,
        adan_state=ctypes.addressof(keep["state"]), adan_hparams=ctypes.addressof(keep["hp"]),
        decay=0.8, eps=1e-5, commitment_weight=1.0, loss=d, workspace=d,
        workspace_bytes=lib.gsvc_quant_train_workspace_bytes(n), train_workspace=d,
        train_workspace_bytes=lib.gsvc_train_step_workspace_bytes(n, 40, 72))
    return lib, a, keep


REFUSALS = [
    # (fields to set, status, part of the message)
    (dict(xyz=None), 1, b"parameter"),
    (dict(features=None), 1, b"parameter"),
    (dict(beta=None), 1, b"scale / beta"),
    (dict(embed_avg=None), 1, b"codebooks"),
    (dict(cholesky_bound=None), 1, b"cholesky_bound"),
    (dict(background=None), 1, b"background"),
    (dict(gt=None), 1, b"gt"),
    (dict(adan_hparams=None), 1, b"hyper-parameters"),
    (dict(adan_state=None), 1, b"Adan state"),
    (dict(loss=None), 1, b"loss"),
    (dict(num_points=0), 1, b"num_points"),
    (dict(num_points=-3), 1, b"num_points"),
    (dict(p_xyz=16), 1, b"go together"),
    (dict(p_xyz=16, p_features=16), 1, b"go together"),
    (dict(loss_kind=2), 1, b"loss_kind"),
    (dict(img_width=0), 1, b"sizes"),
    (dict(flags=0x80), 1, b"flags"),
    (dict(decay=1.5), 1, b"decay"),
    (dict(workspace=None), 2, b"workspace"),
    (dict(workspace_bytes=64), 2, b"workspace"),
    (dict(train_workspace_bytes=64), 2, b"train workspace"),
    (dict(flags=0x4000), 2, b"det_workspace"),
]


@pytest.mark.parametrize("fields,status,msg", REFUSALS, ids=[str(sorted(r[0])) + str(i) for i, r in
                                                             enumerate(REFUSALS)])
def test_entry_refusals_without_launch(fields, status, msg):
    lib, a, keep = _dummy_args()
    for k, v in fields.items():
        setattr(a, k, v)
    assert lib.gsvc_quant_train_step(ctypes.byref(a)) == status
    assert msg in lib.gsvc_last_error(), lib.gsvc_last_error()


def test_entry_refuses_a_missing_state_tensor_and_null():
    lib, a, keep = _dummy_args()
    keep["state"][13] = None
    assert lib.gsvc_quant_train_step(ctypes.byref(a)) == 1
    assert b"Adan state tensor" in lib.gsvc_last_error()
    assert lib.gsvc_quant_train_step(None) == 1 and b"null" in lib.gsvc_last_error()
    # the quantizer half alone: the same checks, and its two inputs
    lib, a, keep = _dummy_args()
    assert lib.gsvc_quant_adan_step(ctypes.byref(a), None, None, None) == 1
    assert b"grad_records" in lib.gsvc_last_error()
    a.num_points = 0
    assert lib.gsvc_quant_adan_step(ctypes.byref(a), 16, 16, None) == 1
    assert b"num_points" in lib.gsvc_last_error()
    a.num_points, a.workspace_bytes = 10, 8
    assert lib.gsvc_quant_adan_step(ctypes.byref(a), 16, 16, None) == 2


def _cpu_model(**kw):
    from gsvc_amd import compress as C
    args = dict(num_points=20, H=40, W=72, BLOCK_H=16, BLOCK_W=16, device="cpu", lr=1e-3, quantize=True,
                opt_type="adan")
    loss_type = kw.pop("loss_type", "L2")
    args.update(kw)
    torch.manual_seed(0)
    m = C.GaussianVideoFrameQ(loss_type=loss_type, **args)
    if args["quantize"]:
        m._init_data()
    return m.train()


@pytest.mark.parametrize("kw,exc,msg", [
    (dict(), RuntimeError, "CPU"),
    (dict(quantize=False), RuntimeError, "quantize=False"),
    (dict(opt_type="adam"), ValueError, "Adan"),
    (dict(loss_type="Fusion1"), ValueError, "L2 and L1"),
    (dict(BLOCK_H=8, BLOCK_W=8), ValueError, "16x16"),
], ids=["cpu", "unquantized", "adam", "fusion1", "blocks"])
def test_fused_method_raises_and_changes_nothing(kw, exc, msg):
    m = _cpu_model(**kw)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    gt = torch.rand(1, 3, 40, 72)
    with pytest.raises(exc, match=msg):
        m.train_iter_quantize_fused(gt)
    after = m.state_dict()
    assert set(before) == set(after)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert len(m.optimizer.state) == 0
    assert m.optimizer.param_groups[0].get("step", 0) == 0
    assert m.scheduler.last_epoch == 0
    if m.quantize:
        assert not bool(m.features_dc_quantizer.initted)  # no k-means ran either


def test_compress_video_fused_raises_on_cpu():
    from gsvc_amd import compress as C
    sd = {"frame_1": {"_xyz": torch.zeros(8, 2), "_cholesky": torch.rand(8, 3),
                      "_features_dc": torch.rand(8, 3)}}
    with pytest.raises(RuntimeError, match="CPU"):
        C.compress_video(sd, [torch.rand(1, 3, 40, 72)], iterations=1, device="cpu", fused=True)


_worst = {}


@pytest.mark.parametrize("n,delta", [(n, d) for n in QT.SIZES for d in (False, True)]
                         + [(QT.BIG, False)])  # the large size has one case, a key frame
def test_ema_restatement_agrees_with_torch(n, delta):
    """The torch ema_update (fp32, CPU) against the float64 restatement: the
    member counts exactly, cluster_size within its two roundings, embed_avg and
    the codebooks within the any-order summation bound (quant_train_cases
    ema_bounds).  Prints the fp32 error in units of each tensor's largest
    element: the figure the GPU test's bar is 4 x of."""
    from gsvc_amd.quantize import ResidualVQ8
    h = QT.half_case(n, delta, 2)
    case = h["case"]
    codes = Q.ref_forward(case)["codes_rgb"]
    ref = QT.ema_ref64(case["feat"], codes, case["cb"], h["cluster"], h["embed"])
    vq = ResidualVQ8(decay=QT.DECAY, eps=QT.EPS)
    vq.codebooks.copy_(torch.from_numpy(case["cb"]))
    vq.cluster_size.copy_(torch.from_numpy(h["cluster"]))
    vq.embed_avg.copy_(torch.from_numpy(h["embed"]))
    vq.ema_update(torch.from_numpy(case["feat"]), torch.from_numpy(codes))
    assert int(ref["counts"][0].sum()) == n == int(ref["counts"][1].sum())
    cs = vq.cluster_size.numpy()
    assert (np.abs(cs - ref["cluster_size"]) <= 3 * QT.U * np.abs(ref["cluster_size"])).all()
    exact = np.array_equal(cs, QT.cluster_size_f32(h["cluster"], ref["counts"]))
    embed_err, cb_err = QT.ema_bounds(ref, n, h["cluster"], h["embed"])
    e_em = np.abs(vq.embed_avg.numpy() - ref["embed_avg"])
    e_cb = np.abs(vq.codebooks.numpy() - ref["codebooks"])
    assert (e_em <= embed_err).all(), (e_em.max(), embed_err.max())
    assert (e_cb <= cb_err).all(), (e_cb.max(), cb_err.max())
    r_em = QT.rel_err(vq.embed_avg.numpy(), ref["embed_avg"])
    r_cb = QT.rel_err(vq.codebooks.numpy(), ref["codebooks"])
    _worst["embed_avg"] = max(_worst.get("embed_avg", 0.0), r_em)
    _worst["codebooks"] = max(_worst.get("codebooks", 0.0), r_cb)
    print(f"ema_update fp32 vs float64, N={n} delta={delta}: embed_avg {r_em:.3e} codebooks {r_cb:.3e} "
          f"of the largest element (cluster_size two-rounding form exact: {exact}); worst so far "
          f"{_worst}")
