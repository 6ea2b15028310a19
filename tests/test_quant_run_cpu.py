"""CPU: ``gsvc_quant_train_run`` is declared, exported and bound, its argument
struct's ctypes mirror matches the header, the entry refuses bad arguments
before any launch, ``train_run_quantize_fused`` raises where it cannot run and
changes nothing, and ``compress_video`` refuses ``run=`` without ``fused``."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

import quant_train_cases as QT
from conftest import REPO

HEADER = os.path.join(REPO, "include", "gsvc_amd.h")
DET = 0x4000  # GSVC_TRAIN_DETERMINISTIC


def test_symbol_and_abi():
    from gsvc_amd import _lib
    assert "gsvc_quant_train_run" in _lib.symbols()
    lib = _lib.load()
    assert hasattr(lib, "gsvc_quant_train_run")
    assert lib.gsvc_quant_train_run.argtypes == [ctypes.c_void_p]
    assert lib.gsvc_abi_version() == _lib.ABI_VERSION == 4
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "gsvc_quant_train_run")
    assert f"#define GSVC_TRAIN_DETERMINISTIC 0x{DET:x}" in open(HEADER).read()


def test_run_args_struct_layout(tmp_path):
    """compress._QuantRunArgs mirrors gsvc_quant_train_run_args field by field."""
    from gsvc_amd.compress import _QuantRunArgs
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    names = [f[0] for f in _QuantRunArgs._fields_]
    assert names == ["step", "iterations", "adan_hparams", "flags", "loss_log", "best_mse", "best_iter",
                     "iter_base", "best_xyz", "best_cholesky", "best_features", "best_scale", "best_beta",
                     "best_codebooks", "best_cluster_size", "best_embed_avg"]
    body = "".join(f'printf("%zu ", offsetof(gsvc_quant_train_run_args, {n}));' for n in names)
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){%s'
                   'printf("%%zu\\n", sizeof(gsvc_quant_train_run_args));return 0;}\n' % (HEADER, body))
    exe = tmp_path / "off"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert got[:-1] == [getattr(_QuantRunArgs, n).offset for n in names]
    assert got[-1] == ctypes.sizeof(_QuantRunArgs)


BEST = ["best_mse", "best_iter", "best_xyz", "best_cholesky", "best_features", "best_scale", "best_beta",
        "best_codebooks", "best_cluster_size", "best_embed_avg"]


def _dummy_run(k=3, n=10):
    """Arguments that pass every check up to the stream's: the device pointers
    are never dereferenced, a failing check returns first."""
    from gsvc_amd import _lib
    from gsvc_amd.compress import _QuantRunArgs
    lib = _lib.load()
    d = 16
    keep = dict(state=(ctypes.c_void_p * 20)(*([d] * 20)), hp=(ctypes.c_double * 10)(*QT.hparams(1)),
                rows=(ctypes.c_double * (10 * k))(*(QT.hparams(1) * k)), flags=(ctypes.c_int * k)())
    a = QT.args_struct(
        n, xyz=d, cholesky=d, features=d, scale=d, beta=d, codebooks=d, cluster_size=d, embed_avg=d,
        cholesky_bound=d, background=d, gt=d, img_height=40, img_width=72, loss_kind=0,
        adan_state=ctypes.addressof(keep["state"]), adan_hparams=ctypes.addressof(keep["hp"]),
        decay=0.8, eps=1e-5, commitment_weight=1.0, loss=d, workspace=d,
        workspace_bytes=lib.gsvc_quant_train_workspace_bytes(n), train_workspace=d,
        train_workspace_bytes=lib.gsvc_train_step_workspace_bytes(n, 40, 72))
    keep["step"] = a
    r = _QuantRunArgs()
    r.step = ctypes.addressof(a)
    r.iterations = k
    r.adan_hparams = ctypes.addressof(keep["rows"])
    r.flags = ctypes.addressof(keep["flags"])
    r.loss_log = d
    return lib, r, keep


RUN_REFUSALS = [
    # (run fields, step fields, flags per iteration or None, status, part of the message)
    (dict(step=None), {}, None, 1, b"null step"),
    (dict(iterations=0), {}, None, 1, b"iterations"),
    (dict(iterations=-2), {}, None, 1, b"iterations"),
    (dict(adan_hparams=None), {}, None, 1, b"adan_hparams"),
    (dict(flags=None), {}, None, 1, b"flags"),
    (dict(loss_log=None), {}, None, 1, b"loss_log"),
    (dict(best_mse=16), {}, None, 1, b"go together"),
    (dict(best_xyz=16, best_embed_avg=16), {}, None, 1, b"go together"),
    ({k: 16 for k in BEST if k != "best_iter"}, {}, None, 1, b"go together"),
    ({k: 16 for k in BEST if k != "best_scale"}, {}, None, 1, b"go together"),
    ({}, dict(grads_out=16), None, 1, b"grads_out"),
    ({}, {}, [0, DET, 0], 1, b"DETERMINISTIC differs"),
    ({}, {}, [DET, DET, 0], 1, b"DETERMINISTIC differs"),
    # the single step's own checks reach the run, per iteration's flags
    ({}, dict(xyz=None), None, 1, b"parameter"),
    ({}, dict(gt=None), None, 1, b"gt"),
    ({}, dict(p_xyz=16), None, 1, b"go together"),
    ({}, {}, [0, 0, 0x80], 1, b"flags"),
    ({}, dict(workspace_bytes=64), None, 2, b"workspace"),
    ({}, {}, [DET, DET, DET], 2, b"det_workspace"),
]


@pytest.mark.parametrize("run_fields,step_fields,flags,status,msg", RUN_REFUSALS,
                         ids=[f"{i}-{r[4].decode().replace(' ', '_')}" for i, r in enumerate(RUN_REFUSALS)])
def test_run_refusals_without_launch(run_fields, step_fields, flags, status, msg):
    lib, r, keep = _dummy_run()
    for k, v in run_fields.items():
        setattr(r, k, v)
    for k, v in step_fields.items():
        setattr(keep["step"], k, v)
    if flags is not None:
        keep["flags"][:] = flags
    assert lib.gsvc_quant_train_run(ctypes.byref(r)) == status
    err = lib.gsvc_last_error()
    assert msg in err and b"quant_train_run" in err, err


def test_run_refuses_null():
    from gsvc_amd import _lib
    lib = _lib.load()
    assert lib.gsvc_quant_train_run(None) == 1
    assert b"null run" in lib.gsvc_last_error()


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
def test_run_method_raises_and_changes_nothing(kw, exc, msg):
    m = _cpu_model(**kw)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    gt = torch.rand(1, 3, 40, 72)
    with pytest.raises(exc, match=msg):
        m.train_run_quantize_fused(gt, 4)
    after = m.state_dict()
    assert set(before) == set(after)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert len(m.optimizer.state) == 0
    assert m.optimizer.param_groups[0].get("step", 0) == 0
    assert m.scheduler.last_epoch == 0
    if m.quantize:
        assert not bool(m.features_dc_quantizer.initted)  # no k-means ran either


def test_compress_video_run_needs_fused():
    from gsvc_amd import compress as C
    sd = {"frame_1": {"_xyz": torch.zeros(8, 2), "_cholesky": torch.rand(8, 3),
                      "_features_dc": torch.rand(8, 3)}}
    frames = [torch.rand(1, 3, 40, 72)]
    with pytest.raises(ValueError, match="fused=True"):
        C.compress_video(sd, frames, iterations=1, device="cpu", run=4)
    with pytest.raises(ValueError, match="run = 0"):
        C.compress_video(sd, frames, iterations=1, device="cpu", fused=True, run=0)
    with pytest.raises(RuntimeError, match="CPU"):  # the run method's own refusal
        C.compress_video(sd, frames, iterations=1, device="cpu", fused=True, run=4)


def test_cli_run_option_reaches_compress_video(tmp_path):
    """``codec encode --run K`` is compress_video's ``run=``: without --fused it is refused."""
    import numpy as np
    from gsvc_amd import codec
    h = w = 32
    (tmp_path / "src.yuv").write_bytes(np.full(h * w * 3 // 2, 90, np.uint8).tobytes())
    torch.save({"frame_1": {"_xyz": torch.zeros(8, 2), "_cholesky": torch.rand(8, 3),
                            "_features_dc": torch.rand(8, 3)}}, tmp_path / "models.pth")
    argv = ["encode", str(tmp_path / "models.pth"), str(tmp_path / "src.yuv"), str(tmp_path / "v.gsvf"),
            "--width", str(w), "--height", str(h), "--iterations", "1", "--device", "cpu", "--run", "4"]
    with pytest.raises(ValueError, match="fused=True"):
        codec.main(argv)
    with pytest.raises(RuntimeError, match="CPU"):
        codec.main(argv + ["--fused"])
