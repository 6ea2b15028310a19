"""Compression stage: quantized frame models, the packed stream, its decoder.

``GaussianVideoFrameQ`` / ``GaussianVideoDelta`` mirror ``GaussianVideo_frame``
/ ``GaussianVideo_delta`` of the reference's GaussianSplats_Compress.py:11-193:
the same parameters and buffers, ``forward``, ``forward_quantize``,
``train_iter_quantize`` and ``_init_data``.  An overfit frame model is
fine-tuned under quantization -- positions through fp16, Cholesky entries
through a learned 6-bit uniform quantizer, colours through a 2-stage residual
VQ -- and a non-key frame is a delta on the previous frame's parameters.  The
quantization itself is one kernel each way (``quantize.quantize_params``); the
render and its backward are the existing operators, the optimizer the existing
``Adan``.  ``train_iter_quantize_fused`` is the same iteration as ONE C call
(``gsvc_quant_train_step``, csrc/quant_train.hip): the quantizer forward, the
fused step's render / loss / backward, the quantizer's backward, Adan on all
five parameters and the codebooks' moving average, with the model's ``Adan``
object still the owner of the state, so the two methods interleave freely.

``encode_frame`` writes a model as the fixed-length stream of
include/gsvc_amd.h (256-byte header + 7 bytes per splat) or, with
``entropy=True``, as its entropy-coded transcoding (version 2, ans.py);
``decode_frames`` turns a list of such streams, of either version, into images
with one expand and one unpack launch and ``render_frames_sum``; ``compress_video`` is the loop of
train_video_Compress.py:240-271 without its image and video writing.
"""
from __future__ import annotations

import copy
import ctypes
import math
import struct
from collections import namedtuple
from typing import List, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from . import ans
from . import train as T
from .adan import Adan
from .frame import loss_fn
from .project_gaussians_2d import project_gaussians_2d
from .ans import entropy_code, entropy_expand
from .quantize import (FakeQuantizationHalf, ResidualVQ8, UniformQuantizer, fixed_bits,
                       quantize_params, vq_loss_from_sums, zeroth_order_bits, _table_bits)
from .rasterize_sum import rasterize_gaussians_sum
from .render import render_frame_sum, render_frames_sum

STREAM_MAGIC = 0x51565347  # "GSVQ"
STREAM_VERSION = 1
STREAM_VERSION_CODED = 2  # the entropy-coded transcoding of version 1 (ans.py)
HEADER_BYTES = 256
SPLAT_BYTES = 7
_HEADER = struct.Struct("<IIiIII3f3f48f")  # magic, version, N, H, W, flags, scale, beta, codebooks
FLAG_DELTA = 1

# unit_bit entry of one parameter group: the bits the packed stream writes, and
# an estimate of what an entropy coder would (None in training mode)
Bits = namedtuple("Bits", ["fixed", "entropy_estimate"])


class _QuantStepArgs(ctypes.Structure):
    """include/gsvc_amd.h gsvc_quant_train_args."""
    _fields_ = [("num_points", ctypes.c_int), ("xyz", ctypes.c_void_p),
                ("cholesky", ctypes.c_void_p), ("features", ctypes.c_void_p),
                ("scale", ctypes.c_void_p), ("beta", ctypes.c_void_p),
                ("codebooks", ctypes.c_void_p), ("cluster_size", ctypes.c_void_p),
                ("embed_avg", ctypes.c_void_p), ("cholesky_bound", ctypes.c_void_p),
                ("p_xyz", ctypes.c_void_p), ("p_cholesky", ctypes.c_void_p),
                ("p_features", ctypes.c_void_p), ("background", ctypes.c_void_p),
                ("gt", ctypes.c_void_p), ("img_height", ctypes.c_uint), ("img_width", ctypes.c_uint),
                ("loss_kind", ctypes.c_int), ("frame_index", ctypes.c_int),
                ("adan_state", ctypes.c_void_p), ("adan_hparams", ctypes.c_void_p),
                ("flags", ctypes.c_int), ("decay", ctypes.c_double), ("eps", ctypes.c_double),
                ("commitment_weight", ctypes.c_double), ("loss", ctypes.c_void_p),
                ("render_out", ctypes.c_void_p), ("grads_out", ctypes.c_void_p),
                ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t),
                ("train_workspace", ctypes.c_void_p), ("train_workspace_bytes", ctypes.c_size_t),
                ("det_workspace", ctypes.c_void_p), ("det_workspace_bytes", ctypes.c_size_t),
                ("det_capacity", ctypes.c_longlong), ("stream", ctypes.c_void_p),
                ("loss_yuv", ctypes.c_void_p), ("loss_chroma", ctypes.c_int)]


class _QuantRunArgs(ctypes.Structure):
    """include/gsvc_amd.h gsvc_quant_train_run_args."""
    _fields_ = [("step", ctypes.c_void_p), ("iterations", ctypes.c_int),
                ("adan_hparams", ctypes.c_void_p), ("flags", ctypes.c_void_p),
                ("loss_log", ctypes.c_void_p), ("best_mse", ctypes.c_void_p),
                ("best_iter", ctypes.c_void_p), ("iter_base", ctypes.c_int),
                ("best_xyz", ctypes.c_void_p), ("best_cholesky", ctypes.c_void_p),
                ("best_features", ctypes.c_void_p), ("best_scale", ctypes.c_void_p),
                ("best_beta", ctypes.c_void_p), ("best_codebooks", ctypes.c_void_p),
                ("best_cluster_size", ctypes.c_void_p), ("best_embed_avg", ctypes.c_void_p)]


_data_ptr = torch.Tensor.data_ptr


class BoundQuantStep:
    """``gsvc_quant_train_step`` bound to a model's tensors (parameters, the
    quantizers' tables, the previous frame's buffers, the 20 Adan state
    tensors): the argument struct, the step's workspace and the four host
    loss words are made once; a call sets the target, the frame parity, the
    hyper-parameters, flags and stream (``train.BoundStep`` is the model).  The
    owner rebuilds it when a bound tensor object or storage changes."""

    def __init__(self, params, tables, bound, prev, background, H, W, loss_type, vq, state, *,
                 yuv_loss=None):
        xyz, chol, feat, scale, beta = params
        self.loss_type, self.yuv_loss = loss_type, yuv_loss  # (the owner rebuilds when either changes)
        n = xyz.shape[0]
        self.tensors = (*params, *tables, bound, *(prev or ()), background, *state)
        self.ids = tuple(map(id, self.tensors))
        self.ptrs = list(map(_data_ptr, self.tensors))
        self.n, self.H, self.W, self.dev = n, int(H), int(W), xyz.device
        self.state = (ctypes.c_void_p * 20)()
        numels = [2 * n, 3 * n, 3 * n, 3, 3]
        for k, t in enumerate(state):
            self.state[k] = T._f32_ptr(t, "adan_state", numels[k // 4])
        self.hp = (ctypes.c_double * 10)()
        self.lib = L.load()
        self.ws = torch.empty((int(self.lib.gsvc_quant_train_workspace_bytes(n)),), dtype=torch.uint8,
                              device=self.dev)
        self.host = self.lib.gsvc_host_alloc(16)
        if not self.host:
            raise RuntimeError(self.lib.gsvc_last_error().decode(errors="replace"))
        self.host_f = (ctypes.c_float * 4).from_address(self.host)
        a = self.args = _QuantStepArgs()
        a.num_points = n
        a.xyz, a.cholesky = T._f32_ptr(xyz, "_xyz", 2 * n), T._f32_ptr(chol, "_cholesky", 3 * n)
        a.features = T._f32_ptr(feat, "_features_dc", 3 * n)
        a.scale, a.beta = T._f32_ptr(scale, "scale", 3), T._f32_ptr(beta, "beta", 3)
        a.codebooks = T._f32_ptr(tables[0], "codebooks", 48)
        a.cluster_size = T._f32_ptr(tables[1], "cluster_size", 16)
        a.embed_avg = T._f32_ptr(tables[2], "embed_avg", 48)
        a.cholesky_bound = T._f32_ptr(bound, "cholesky_bound", 3)
        if prev is not None:
            a.p_xyz = T._f32_ptr(prev[0], "p_xyz", 2 * n)
            a.p_cholesky = T._f32_ptr(prev[1], "p_cholesky", 3 * n)
            a.p_features = T._f32_ptr(prev[2], "p_features_dc", 3 * n)
        a.background = T._f32_ptr(background, "background", 3)
        a.img_height, a.img_width = self.H, self.W
        self.loss_words = T.loss_args(a, loss_type, yuv_loss, self.H, self.W)
        a.adan_state = ctypes.addressof(self.state)
        a.adan_hparams = ctypes.addressof(self.hp)
        a.decay, a.eps, a.commitment_weight = vq.decay, vq.eps, vq.commitment_weight
        self.vq_scalars = (vq.decay, vq.eps, vq.commitment_weight)
        a.loss = self.host
        a.workspace, a.workspace_bytes = self.ws.data_ptr(), self.ws.numel()
        self.args_ref = ctypes.byref(a)
        self.fn = self.lib.gsvc_quant_train_step
        # gsvc_quant_train_run: its arguments, and host arrays for run_cap iterations
        self.run_args = _QuantRunArgs()
        self.run_args.step = ctypes.addressof(a)
        self.run_cap, self.run_host = 0, None
        self.run_hp = self.run_flags = self.run_log = None

    def __del__(self):
        for name in ("host", "run_host"):
            if getattr(self, name, None):
                try:
                    self.lib.gsvc_host_free(getattr(self, name))
                except Exception:  # interpreter shutdown
                    pass
                setattr(self, name, None)

    def __deepcopy__(self, memo):
        return None  # a copied model binds its own tensors on its first step

    def matches(self, tensors, vq) -> bool:
        return (tuple(map(id, tensors)) == self.ids and list(map(_data_ptr, tensors)) == self.ptrs
                and (vq.decay, vq.eps, vq.commitment_weight) == self.vq_scalars)

    def step(self, gt, hparams, flags, render_out=None, grads_out=None, sync=True):
        """One call and one read-back: (mse, mae, commitment sum 0, 1).
        ``sync=False`` (tools' timing) only enqueues the call and returns None."""
        if not (gt.is_cuda and gt.dtype is torch.float32 and gt.is_contiguous()
                and gt.numel() == 3 * self.H * self.W):
            raise RuntimeError("gt must be a contiguous float32 CUDA tensor of 3*H*W elements")
        a = self.args
        for k, x in enumerate(hparams):
            self.hp[k] = x
        # train.py's workspace of this stream: zeroed counters, the frame parity
        ws = T._workspace(self.dev, self.n, self.H, self.W)
        if ws.pending is not None:  # a bound step's work enqueued ahead: not for this call
            ws.dirty = True
            ws = T._workspace(self.dev, self.n, self.H, self.W)
        if torch.are_deterministic_algorithms_enabled():
            buf, cap = ws.det_workspace(self.dev, self.n, 16 * self.n)
            a.det_workspace, a.det_workspace_bytes, a.det_capacity = buf.data_ptr(), buf.numel(), cap
            flags |= T.TRAIN_DETERMINISTIC
        else:
            a.det_workspace, a.det_workspace_bytes, a.det_capacity = None, 0, 0
        a.gt = gt.data_ptr()
        a.frame_index = ws.frame
        a.flags = flags
        a.render_out = T._f32_ptr(render_out, "render_out", 3 * self.H * self.W) or None
        a.grads_out = T._f32_ptr(grads_out, "grads_out", 8 * self.n + 6) or None
        a.train_workspace, a.train_workspace_bytes = ws.buf_ptr, ws.buf.numel()
        stream = T._raw_stream(self.dev.index)
        a.stream = stream
        T._note_launch(a.xyz)
        rc = self.fn(self.args_ref)
        if rc != 0:
            ws.dirty = True
            msg = self.lib.gsvc_last_error().decode(errors="replace")
            raise RuntimeError(f"gsvc_quant_train_step failed (status {rc}): {msg}")
        ws.frame += 1
        if not sync:
            return None
        rc = self.lib.gsvc_stream_sync(stream)  # the reference's PSNR .item()
        if rc != 0:
            ws.dirty = True
            msg = self.lib.gsvc_last_error().decode(errors="replace")
            raise RuntimeError(f"gsvc_quant_train_step failed (status {rc}): {msg}")
        return tuple(self.host_f)

    def _run_room(self, k: int) -> None:
        """Host arrays for a run of ``k`` iterations: hyper-parameters, flags and
        the pinned loss log (kept, and grown when a longer run comes)."""
        if k <= self.run_cap:
            return
        host = self.lib.gsvc_host_alloc(16 * k)
        if not host:
            raise RuntimeError(self.lib.gsvc_last_error().decode(errors="replace"))
        if self.run_host:
            self.lib.gsvc_host_free(self.run_host)
        self.run_host, self.run_cap = host, k
        self.run_log = (ctypes.c_float * (4 * k)).from_address(host)
        self.run_hp = (ctypes.c_double * (10 * k))()
        self.run_flags = (ctypes.c_int * k)()
        r = self.run_args
        r.adan_hparams = ctypes.addressof(self.run_hp)
        r.flags = ctypes.addressof(self.run_flags)
        r.loss_log = host

    def run(self, gt, rows, flags, best=None, iter_base=0):
        """``gsvc_quant_train_run`` over ``len(rows)`` iterations: one call and
        one wait; per iteration its four loss words.  ``rows[i]`` are iteration
        i's ten hyper-parameters, ``flags[i]`` its flags; ``best`` the ten
        device tensors of the best-state block (``QuantBestState``)."""
        if not (gt.is_cuda and gt.dtype is torch.float32 and gt.is_contiguous()
                and gt.numel() == 3 * self.H * self.W):
            raise RuntimeError("gt must be a contiguous float32 CUDA tensor of 3*H*W elements")
        k = len(rows)
        self._run_room(k)
        a, r = self.args, self.run_args
        ws = T._workspace(self.dev, self.n, self.H, self.W)
        if ws.pending is not None:  # a bound step's work enqueued ahead: not for this call
            ws.dirty = True
            ws = T._workspace(self.dev, self.n, self.H, self.W)
        det = 0
        if torch.are_deterministic_algorithms_enabled():
            buf, cap = ws.det_workspace(self.dev, self.n, 16 * self.n)
            a.det_workspace, a.det_workspace_bytes, a.det_capacity = buf.data_ptr(), buf.numel(), cap
            det = T.TRAIN_DETERMINISTIC
        else:
            a.det_workspace, a.det_workspace_bytes, a.det_capacity = None, 0, 0
        for i in range(k):
            self.run_hp[10 * i:10 * i + 10] = rows[i]
            self.run_flags[i] = flags[i] | det
        a.gt = gt.data_ptr()
        a.frame_index = ws.frame
        a.flags = self.run_flags[0]
        a.render_out = a.grads_out = None
        a.train_workspace, a.train_workspace_bytes = ws.buf_ptr, ws.buf.numel()
        stream = T._raw_stream(self.dev.index)
        a.stream = stream
        r.iterations = k
        names = [f[0] for f in _QuantRunArgs._fields_]
        if best is None:
            for name in names[5:7] + names[8:]:
                setattr(r, name, None)
            r.iter_base = 0
        else:
            n = self.n
            r.best_mse = T._f32_ptr(best[0], "best_mse", 1)
            if best[1].dtype is not torch.int32 or best[1].numel() != 1 or not best[1].is_cuda:
                raise RuntimeError("best_iter must be one int32 on the device")
            r.best_iter = best[1].data_ptr()
            for name, t, numel in zip(names[8:], best[2:], (2 * n, 3 * n, 3 * n, 3, 3, 48, 16, 48)):
                setattr(r, name, T._f32_ptr(t, name, numel))
            r.iter_base = iter_base
        T._note_launch(a.xyz)
        rc = self.lib.gsvc_quant_train_run(ctypes.byref(r))
        if rc == 0:
            ws.frame += k
            rc = self.lib.gsvc_stream_sync(stream)
        if rc != 0:
            ws.dirty = True
            msg = self.lib.gsvc_last_error().decode(errors="replace")
            raise RuntimeError(f"gsvc_quant_train_run failed (status {rc}): {msg}")
        words = list(self.run_log[:4 * k])
        return [tuple(words[4 * i:4 * i + 4]) for i in range(k)]


class QuantBestState:
    """The reference's "best state" of a quantized fine-tune
    (train_video_Compress.py:89-102), kept on the device by
    ``train_run_quantize_fused``: snapshots of the eight tensors an iteration
    changes (the three parameters, the Cholesky quantizer's scale and beta, the
    codebooks with their moving averages), the best mean squared error and its
    iteration.  It counts the iterations it has seen: an iteration's index is
    global over the runs it was passed to."""

    def __init__(self, model):
        self.seen = 0
        with torch.no_grad():
            self.snapshot = [torch.empty_like(t) for t in self._tensors(model)]
            dev = model._xyz.device
            self.best_mse = torch.full((1,), math.inf, dtype=torch.float32, device=dev)
            self.best_iter = torch.full((1,), -1, dtype=torch.int32, device=dev)

    @staticmethod
    def _tensors(model):
        uq, vq = model.cholesky_quantizer, model.features_dc_quantizer
        return [model._xyz, model._cholesky, model._features_dc, uq.scale, uq.beta, vq.codebooks,
                vq.cluster_size, vq.embed_avg]

    def tensors(self):
        """What ``BoundQuantStep.run`` passes: the two scalars, the snapshots."""
        return [self.best_mse, self.best_iter, *self.snapshot]

    @property
    def index(self) -> int:
        """Global index of the best iteration; -1 when none has taken."""
        return int(self.best_iter.item())

    @property
    def mse(self) -> float:
        return float(self.best_mse.item())

    def load_into(self, model) -> bool:
        """Write the snapshot back into ``model``: its ``state_dict()`` is then
        what the host loop's ``best_sd`` holds.  False, and nothing written,
        when no iteration has taken."""
        if self.index == -1:
            return False
        with torch.no_grad():
            for dst, src in zip(self._tensors(model), self.snapshot):
                if dst.shape != src.shape:
                    raise ValueError("QuantBestState.load_into: the model's shapes differ from "
                                     "the snapshot's")
                dst.copy_(src)
        T.bump_param_epoch()
        return True


class _QuantFrame(nn.Module):
    """What the key-frame and delta models share."""
    _delta = False

    def __init__(self, loss_type="L2", **kwargs):
        super().__init__()
        self.loss_type = loss_type
        # loss_type "YUV": the weighted Y/U/V loss's spec (video.YuvLoss; None: YuvLoss())
        self.yuv_loss = kwargs.get("yuv_loss")
        if loss_type == "YUV":
            if self.yuv_loss is None:
                from .video import YuvLoss
                self.yuv_loss = YuvLoss()
            self.yuv_loss.check_size(kwargs["H"], kwargs["W"])
        self.init_num_points = n = kwargs["num_points"]
        self.H, self.W = kwargs["H"], kwargs["W"]
        self.BLOCK_W, self.BLOCK_H = kwargs["BLOCK_W"], kwargs["BLOCK_H"]
        self.tile_bounds = ((self.W + self.BLOCK_W - 1) // self.BLOCK_W,
                            (self.H + self.BLOCK_H - 1) // self.BLOCK_H, 1)
        self.device = kwargs["device"]
        self._xyz = nn.Parameter(torch.atanh(2 * (torch.rand(n, 2) - 0.5)))
        self._cholesky = nn.Parameter(torch.rand(n, 3))
        self._features_dc = nn.Parameter(torch.rand(n, 3))
        self.last_size = (self.H, self.W)
        if self._delta:
            self.register_buffer("p_xyz", torch.atanh(2 * (torch.rand(n, 2) - 0.5)))
            self.register_buffer("p_cholesky", torch.rand(n, 3))
            self.register_buffer("p_features_dc", torch.rand(n, 3))
        self.register_buffer("_opacity", torch.ones((n, 1)))
        self.register_buffer("background", torch.ones(3))
        self.register_buffer("bound", torch.tensor([0.5, 0.5]).view(1, 2))
        self.register_buffer("cholesky_bound", torch.tensor([0.5, 0, 0.5]).view(1, 3))
        self.quantize = kwargs["quantize"]
        if self.quantize:
            self.xyz_quantizer = FakeQuantizationHalf.apply
            self.features_dc_quantizer = ResidualVQ8(kmeans_iters=5)
            self.cholesky_quantizer = UniformQuantizer(signed=False, bits=6, learned=True,
                                                       num_channels=3)
        if kwargs.get("opt_type", "adan") == "adam":
            self.optimizer = torch.optim.Adam(self.parameters(), lr=kwargs["lr"])
        else:
            self.optimizer = Adan(self.parameters(), lr=kwargs["lr"])
        self.scheduler = torch.optim.lr_scheduler.StepLR(self.optimizer, step_size=20000, gamma=0.5)

    def _init_data(self):
        self.cholesky_quantizer._init_data(self._cholesky)

    def _prev(self):
        return (self.p_xyz, self.p_cholesky, self.p_features_dc) if self._delta else None

    @property
    def get_xyz(self):
        return torch.tanh(self._xyz + self.p_xyz) if self._delta else torch.tanh(self._xyz)

    @property
    def get_features(self):
        return self._features_dc + self.p_features_dc if self._delta else self._features_dc

    @property
    def get_cholesky_elements(self):
        if self._delta:
            return self._cholesky + self.p_cholesky + self.cholesky_bound
        return self._cholesky + self.cholesky_bound

    def _render(self, means, cholesky_elements, colors):
        self.xys, depths, self.radii, conics, num_tiles_hit = project_gaussians_2d(
            means, cholesky_elements, self.H, self.W, self.tile_bounds)
        out_img = rasterize_gaussians_sum(self.xys, depths, self.radii, conics, num_tiles_hit,
                                          colors, self._opacity, self.H, self.W, self.BLOCK_H,
                                          self.BLOCK_W, background=self.background,
                                          return_alpha=False)
        out_img = torch.clamp(out_img, 0, 1)
        return out_img.view(-1, self.H, self.W, 3).permute(0, 3, 1, 2).contiguous()

    def forward(self):
        """The unquantized render (GaussianSplats_Compress.py:62-69, 157-163)."""
        return {"render": self._render(self.get_xyz, self.get_cholesky_elements, self.get_features)}

    def quantized(self, commit=None):
        """quantize_params of this model: (xq, Lq, cq, codes_chol, codes_rgb,
        commit_sums); initialises the codebooks on first use.  The commitment
        sums are computed in training mode or with autograd on (``commit``
        overrides); otherwise they are None."""
        if commit is None:
            commit = self.training or torch.is_grad_enabled()
        if not self.quantize:
            raise RuntimeError("the model was built with quantize=False")
        vq = self.features_dc_quantizer
        if not vq.is_initted():
            vq.init_codebooks(self._features_dc)
        uq = self.cholesky_quantizer
        return quantize_params(self._xyz, self._cholesky, self._features_dc, uq.scale, uq.beta,
                               vq.codebooks, self.cholesky_bound, self._prev(), commit)

    def forward_quantize(self):
        """GaussianSplats_Compress.py:71-84, 165-179.  ``unit_bit`` lists, for
        positions, Cholesky codes, (unused) and colours, a ``Bits(fixed,
        entropy_estimate)``: the bits ``encode_frame`` writes for the group
        (header fields included: they sum to 8 * len(encode_frame(self))), and
        in eval mode the zeroth-order entropy of the codes plus the table cost
        quantize.py:72-80 counts -- an estimate; the reference's figure comes
        from an ANS coder."""
        n = self._xyz.shape[0]
        vq = self.features_dc_quantizer
        xq, Lq, cq, codes_chol, codes_rgb, sums = self.quantized()
        if self.training:
            vq.ema_update(self._features_dc, codes_rgb)
        # inference (eval mode, no autograd) skips the commitment sums: the loss is 0 there
        vq_loss = (xq.new_zeros(()) if sums is None
                   else vq_loss_from_sums(sums, n, vq.commitment_weight))
        if (not torch.is_grad_enabled() and xq.is_cuda and self.BLOCK_H == 16 and self.BLOCK_W == 16):
            # inference: the one-call frame render applies tanh itself
            out_img = render_frame_sum(xq, Lq, cq, self.H, self.W, self.background, xyz_tanh=True,
                                       cholesky_bound=None)
        else:
            out_img = self._render(torch.tanh(xq), Lq, cq)
        m_fix, s_fix, c_fix = fixed_bits(n)
        tables = 6 * 32, vq.codebooks.numel() * 32
        misc = 8 * HEADER_BYTES - sum(tables)
        est = [None] * 4
        if not self.training:
            hs, us = zeroth_order_bits(codes_chol.cpu().numpy())
            hc, uc = zeroth_order_bits(codes_rgb.cpu().numpy())
            est = [m_fix, hs + _table_bits(us) + tables[0], 0, hc + _table_bits(uc) + tables[1]]
        unit_bit = [Bits(m_fix + misc, est[0]), Bits(s_fix + tables[0], est[1]), Bits(0, est[2]),
                    Bits(c_fix + tables[1], est[3])]
        return {"render": out_img, "vq_loss": vq_loss, "unit_bit": unit_bit}

    def train_iter_quantize(self, gt_image):
        """GaussianSplats_Compress.py:86-98, 181-193."""
        render_pkg = self.forward_quantize()
        image = render_pkg["render"]
        loss = loss_fn(image.squeeze(0), gt_image.squeeze(0), self.loss_type,
                       lambda_value=0, yuv_loss=self.yuv_loss) + render_pkg["vq_loss"]
        loss.backward()
        with torch.no_grad():
            mse_loss = F.mse_loss(image, gt_image)
            psnr = 10 * math.log10(1.0 / mse_loss.item())
        self.optimizer.step()
        self.optimizer.zero_grad(set_to_none=True)
        self.scheduler.step()
        return loss, psnr

    def _fused_tensors(self, gt_image):
        """The checks of ``train_iter_quantize_fused``; raises with the reason,
        before anything has changed.  Returns the five parameters."""
        if not self.quantize:
            raise RuntimeError("train_iter_quantize_fused: the model was built with quantize=False")
        if self.loss_type not in T.LOSS_KIND:
            raise ValueError("train_iter_quantize_fused supports the L2 and L1 losses and the YUV loss, not "
                             f"{self.loss_type!r}")
        opt = self.optimizer
        if not isinstance(opt, Adan):
            raise ValueError("train_iter_quantize_fused needs the Adan optimizer (opt_type='adan'), "
                             f"not {type(opt).__name__}")
        if self.BLOCK_H != 16 or self.BLOCK_W != 16:
            raise ValueError("train_iter_quantize_fused needs 16x16 blocks, not "
                             f"{self.BLOCK_H}x{self.BLOCK_W}")
        uq = self.cholesky_quantizer
        params = (self._xyz, self._cholesky, self._features_dc, uq.scale, uq.beta)
        if not self._xyz.is_cuda:
            raise RuntimeError("train_iter_quantize_fused: the model is on the CPU; the fused step "
                               "runs on a HIP device only (train_iter_quantize runs anywhere)")
        if opt.defaults["max_grad_norm"] > 0:
            raise ValueError("train_iter_quantize_fused does not clip gradients (max_grad_norm > 0)")
        group = opt.param_groups[0]["params"] if len(opt.param_groups) == 1 else ()
        if len(group) != 5 or {id(p) for p in group} != {id(p) for p in params}:
            raise RuntimeError("train_iter_quantize_fused: the optimizer must hold the model's five "
                               "parameters in one group")
        for p in params:
            if p.grad is not None:
                raise RuntimeError("train_iter_quantize_fused: a parameter has a pending gradient "
                                   "(zero_grad(set_to_none=True) first)")
            if (not p.requires_grad or p.dtype is not torch.float32 or not p.is_contiguous()
                    or p.device != self._xyz.device):
                raise RuntimeError("train_iter_quantize_fused: parameters must be trainable "
                                   "contiguous float32 tensors on one device")
        if gt_image.numel() != 3 * self.H * self.W or gt_image.device != self._xyz.device:
            raise ValueError(f"train_iter_quantize_fused: the target must hold 3 x {self.H} x {self.W} "
                             "elements on the model's device")
        return params

    def _fused_step(self, gt_image, render_out=None, grads_out=None):
        """One ``gsvc_quant_train_step`` with this optimizer's state, step
        counter and learning rate: its four loss words.  With ``grads_out``
        (the test hook) nothing is updated and no counter moves."""
        params = self._fused_tensors(gt_image)
        vq, opt = self.features_dc_quantizer, self.optimizer
        if not vq.is_initted():
            vq.init_codebooks(self._features_dc)
        hook = grads_out is not None
        group = opt.param_groups[0]
        step = group.get("step", 0) + 1
        hparams = self._fused_hparams(group, step)
        state, flags = self._fused_state(params, step, hook)
        bs, gt = self._fused_bound(params, state, gt_image)
        if not hook:
            group["step"] = step
            T.bump_param_epoch()  # work another fused step enqueued ahead is stale now
        return bs.step(gt, hparams, flags, render_out, grads_out)

    @staticmethod
    def _fused_hparams(group, step):
        """The ten hyper-parameters of Adan step ``step`` at the group's learning rate."""
        b1, b2, b3 = group["betas"]
        return [b1, b2, b3, 1.0 - b1 ** step, 1.0 - b2 ** step, math.sqrt(1.0 - b3 ** step),
                group["lr"], group["weight_decay"], group["eps"], 1.0]

    def _fused_state(self, params, step, hook=False):
        """The 20 Adan state tensors, created as ``Adan.step`` would, and the
        flags of step ``step``: no_prox and the first-step bits."""
        opt = self.optimizer
        flags = 1 if opt.param_groups[0]["no_prox"] else 0
        state = []
        for q, p in enumerate(params):
            if hook:  # nothing is read or written: any valid pointers
                state += [p] * 4
                continue
            st = opt.state[p]
            for k in ("exp_avg", "exp_avg_sq", "exp_avg_diff"):  # as Adan.step creates them
                if k not in st:
                    st[k] = torch.zeros_like(p)
            if "neg_pre_grad" not in st or step == 1:
                if "neg_pre_grad" not in st:
                    st["neg_pre_grad"] = torch.zeros_like(p)
                flags |= 1 << (1 + q)  # the kernel starts it at -grad
            state += [st["exp_avg"], st["exp_avg_sq"], st["exp_avg_diff"], st["neg_pre_grad"]]
        return state, flags

    def _fused_bound(self, params, state, gt_image):
        """The ``BoundQuantStep`` of these tensors (rebuilt when one changed) and
        the target as the entry takes it."""
        vq = self.features_dc_quantizer
        gt = gt_image.detach() if gt_image.requires_grad else gt_image
        if gt.dtype is not torch.float32 or not gt.is_contiguous():
            gt = gt.float().contiguous()
        tables = (vq.codebooks, vq.cluster_size, vq.embed_avg)
        bound = (*params, *tables, self.cholesky_bound, *(self._prev() or ()), self.background, *state)
        bs = self.__dict__.get("_bound_quant_step")
        if (bs is None or bs.loss_type != self.loss_type or bs.yuv_loss is not self.yuv_loss
                or not bs.matches(bound, vq)):
            bs = BoundQuantStep(params, tables, self.cholesky_bound, self._prev(), self.background,
                                self.H, self.W, self.loss_type, vq, state, yuv_loss=self.yuv_loss)
            self.__dict__["_bound_quant_step"] = bs
        return bs, gt

    def train_iter_quantize_fused(self, gt_image):
        """``train_iter_quantize`` as one C call (``gsvc_quant_train_step``):
        returns (loss, psnr), the loss a host scalar tensor.  The model's Adan
        object keeps the state, the step counter and the learning rate, and the
        scheduler steps, so this and ``train_iter_quantize`` interleave at any
        iteration.  HIP devices, Adan, 16x16 blocks and the L2 / L1 / YUV losses
        only: anything else raises (nothing falls back to the op-by-op method).
        With the YUV loss the returned loss is that loss plus the VQ term; the
        PSNR is still the RGB one."""
        mse, mae, s0, s1 = self._fused_step(gt_image)
        opt = self.optimizer
        opt._opt_called = True  # the step ran: keeps StepLR's call-order check quiet
        self.scheduler.optimizer._opt_called = True
        self.scheduler.step()
        vq = self.features_dc_quantizer
        n = self._xyz.shape[0]
        loss = torch.empty(())
        loss.numpy()[...] = ((mse if self.loss_type == "L2" else mae)  # (YUV: word 1 is that loss)
                             + vq.commitment_weight * (s0 + s1) / (3 * n))
        psnr = 10 * math.log10(1.0 / mse)
        return loss, psnr

    def train_run_quantize_fused(self, gt_image, iterations, best=None):
        """``iterations`` times ``train_iter_quantize_fused`` as ONE C call
        (``gsvc_quant_train_run``) and one wait: returns (losses, psnrs), per
        iteration what the single-step method returns (the loss as the float
        its fp32 host tensor holds).  The hyper-parameter rows are made on the
        host up front -- the learning rate of each iteration from the
        scheduler, which steps ``iterations`` times -- and nothing in between
        depends on a device result.  ``best`` (a ``QuantBestState``) keeps the
        reference's best state on the device: iteration i of this run has the
        index ``best.seen + i``.  Interleaves with ``train_iter_quantize_fused``
        and ``train_iter_quantize`` at any iteration; the same restrictions,
        raised before anything has changed.  With the YUV loss the losses are
        that loss plus the VQ term, while the best state on the device is still
        chosen by the RGB mean squared error (the PSNR's)."""
        params = self._fused_tensors(gt_image)
        k = int(iterations)
        if k < 1:
            raise ValueError(f"train_run_quantize_fused: iterations = {iterations}, not >= 1")
        if best is not None and not isinstance(best, QuantBestState):
            raise TypeError("train_run_quantize_fused: best must be a QuantBestState")
        vq, opt = self.features_dc_quantizer, self.optimizer
        if not vq.is_initted():
            vq.init_codebooks(self._features_dc)
        group = opt.param_groups[0]
        step0 = group.get("step", 0)
        state, first = self._fused_state(params, step0 + 1)
        bs, gt = self._fused_bound(params, state, gt_image)
        opt._opt_called = True  # keeps StepLR's call-order check quiet
        self.scheduler.optimizer._opt_called = True
        rows, flags = [], []
        for i in range(k):
            rows.append(self._fused_hparams(group, step0 + 1 + i))
            flags.append(first if i == 0 else first & 1)
            self.scheduler.step()
        group["step"] = step0 + k
        T._param_epoch[0] += k  # work another fused step enqueued ahead is stale now
        base = 0 if best is None else best.seen
        words = bs.run(gt, rows, flags, None if best is None else best.tensors(), base)
        if best is not None:
            best.seen += k
        n = self._xyz.shape[0]
        pick = 0 if self.loss_type == "L2" else 1  # (L1, YUV: word 1)
        losses, psnrs = [], []
        for w in words:
            losses.append(float(np.float32(w[pick] + vq.commitment_weight * (w[2] + w[3]) / (3 * n))))
            psnrs.append(10 * math.log10(1.0 / w[0]))
        return losses, psnrs


class GaussianVideoFrameQ(_QuantFrame):
    """A key frame under quantization (GaussianVideo_frame)."""
    _delta = False


class GaussianVideoDelta(_QuantFrame):
    """A non-key frame: quantized deltas on the buffers ``p_xyz``, ``p_cholesky``,
    ``p_features_dc`` (GaussianVideo_delta)."""
    _delta = True


# --------------------------------------------------------------------------
# the packed stream

def _header(n, H, W, delta, scale, beta, codebooks) -> bytes:
    vals = [float(v) for v in scale] + [float(v) for v in beta] + [float(v) for v in codebooks]
    h = _HEADER.pack(STREAM_MAGIC, STREAM_VERSION, n, H, W, FLAG_DELTA if delta else 0, *vals)
    return h + bytes(HEADER_BYTES - len(h))


def parse_header(buf) -> dict:
    """Fields of one frame stream's header, of either version (``version``; a
    version-2 header also gives ``S``, ``n_seg`` and ``payload_bytes``); raises
    ValueError on a wrong magic, version, length or N, and for version 2 on
    whatever ``ans.parse_coded`` refuses."""
    if len(buf) < HEADER_BYTES:
        raise ValueError(f"stream truncated: {len(buf)} bytes, the header is {HEADER_BYTES}")
    f = _HEADER.unpack_from(buf, 0)
    if f[0] != STREAM_MAGIC:
        raise ValueError(f"wrong magic 0x{f[0]:08x}")
    if f[1] not in (STREAM_VERSION, STREAM_VERSION_CODED):
        raise ValueError(f"stream version {f[1]}, not {STREAM_VERSION} or {STREAM_VERSION_CODED}")
    n = f[2]
    extra = {}
    if f[1] == STREAM_VERSION_CODED:
        coded = ans.parse_coded(buf)
        extra = {k: coded[k] for k in ("S", "n_seg", "payload_bytes")}
    elif n < 0 or len(buf) != HEADER_BYTES + SPLAT_BYTES * n:
        raise ValueError(f"stream of {len(buf)} bytes does not hold N = {n} splats")
    return dict(N=n, H=f[3], W=f[4], delta=bool(f[5] & FLAG_DELTA),
                scale=np.array(f[6:9], np.float32), beta=np.array(f[9:12], np.float32),
                codebooks=np.array(f[12:60], np.float32).reshape(2, 8, 3), version=f[1], **extra)


def pack_planes_host(xyz, codes_chol, codes_rgb) -> bytes:
    """The two planes (7 N bytes) from positions and codes, on the host."""
    n = xyz.shape[0]
    a = np.ascontiguousarray(np.asarray(xyz, np.float32).astype("<f2")).tobytes()
    cc = np.asarray(codes_chol).astype(np.uint32) & 63
    cr = np.asarray(codes_rgb).astype(np.uint32) & 7
    w = cc[:, 0] | cc[:, 1] << 6 | cc[:, 2] << 12 | cr[:, 0] << 18 | cr[:, 1] << 21
    b = np.stack([w & 0xff, (w >> 8) & 0xff, (w >> 16) & 0xff], axis=1).astype(np.uint8)
    return a + b.reshape(n * 3).tobytes()


def _frame_parts(model):
    """(header bytes, xyz, codes_chol, codes_rgb) of the model's quantized state."""
    _, _, _, codes_chol, codes_rgb, _ = model.quantized(commit=False)
    xyz = model._xyz.detach().float().contiguous()
    uq, vq = model.cholesky_quantizer, model.features_dc_quantizer
    head = _header(xyz.shape[0], model.H, model.W, model._delta, uq.scale.detach().cpu().tolist(),
                   uq.beta.detach().cpu().tolist(), vq.codebooks.cpu().reshape(-1).tolist())
    return head, xyz, codes_chol, codes_rgb


def encode_frames(models, entropy: bool = False, segment: int = 32) -> List[bytes]:
    """``encode_frame`` of every model of a list.  Models on one HIP device are
    packed into one device buffer (headers uploaded, ``gsvc_pack_splats``
    writing the planes behind them) and, with ``entropy``, coded there in one
    ``gsvc_encode_stream`` call: the F coded lengths are read back once and each
    frame's bytes copied out.  CPU models are packed and coded on the host
    (``ans.entropy_code``); the bytes are the same either way."""
    models = list(models)
    if entropy and not 1 <= int(segment) <= ans.MAX_SEGMENT:
        raise ValueError(f"segment = {segment}, not in 1..{ans.MAX_SEGMENT}")
    with torch.no_grad():
        parts = [_frame_parts(m) for m in models]
        devices = {p[1].device for p in parts}
        if len(devices) > 1:
            return [encode_frames([m], entropy, segment)[0] for m in models]
        if not parts or not parts[0][1].is_cuda:
            v1 = [head + pack_planes_host(xyz.numpy(), cc.numpy(), cr.numpy())
                  for head, xyz, cc, cr in parts]
            return [ans.entropy_code(s, segment) for s in v1] if entropy else v1
        device = parts[0][1].device
        sizes = [p[1].shape[0] for p in parts]
        offs = [0]
        for n in sizes:
            offs.append(offs[-1] + HEADER_BYTES + SPLAT_BYTES * n)
        buf = torch.empty((offs[-1],), dtype=torch.uint8, device=device)
        for o, (head, xyz, cc, cr) in zip(offs, parts):
            buf[o:o + HEADER_BYTES].copy_(torch.frombuffer(bytearray(head), dtype=torch.uint8))
            L.call("gsvc_pack_splats", xyz.shape[0], L.ptr(xyz), L.ptr(cc), L.ptr(cr),
                   ctypes.c_void_p(buf.data_ptr() + o + HEADER_BYTES), L.stream(device))
        if entropy:
            return ans.entropy_code_device(buf, sizes, segment)
        blob = buf.cpu().numpy().tobytes()
        return [blob[a:b] for a, b in zip(offs, offs[1:])]


def encode_frame(model, entropy: bool = False, segment: int = 32) -> bytes:
    """The model's quantized parameters as one frame stream: ``256 + 7 * N``
    bytes, or with ``entropy`` their entropy-coded transcoding in segments of
    ``segment`` splats: ``ans.entropy_code``'s bytes, coded on the device for a
    model on a HIP device (``encode_frames`` with one frame)."""
    return encode_frames([model], entropy, segment)[0]


def unpack_frames_host(streams: Sequence[bytes], cholesky_bound=(0.5, 0.0, 0.5), prev=None):
    """The decoder's arithmetic in numpy: per frame (xq, Lq, cq, Lpre), fp32,
    one rounding per op as in csrc/quant.hip.  ``prev`` = (xq, Lpre, cq) of the
    frame before the first one, for a stream that starts with a delta frame."""
    bound = np.asarray(cholesky_bound, np.float32).reshape(1, 3)
    out = []
    for k, buf in enumerate(streams):
        h = parse_header(buf)
        if h["version"] == STREAM_VERSION_CODED:
            buf = ans.entropy_expand(buf)
        n = h["N"]
        a = np.frombuffer(buf, "<f2", count=2 * n, offset=HEADER_BYTES).reshape(n, 2)
        b = np.frombuffer(buf, np.uint8, count=3 * n, offset=HEADER_BYTES + 4 * n).reshape(n, 3)
        w = b[:, 0].astype(np.uint32) | b[:, 1].astype(np.uint32) << 8 | b[:, 2].astype(np.uint32) << 16
        codes = np.stack([w & 63, (w >> 6) & 63, (w >> 12) & 63], axis=1).astype(np.float32)
        i0, i1 = ((w >> 18) & 7).astype(np.int64), ((w >> 21) & 7).astype(np.int64)
        xq = a.astype(np.float32)
        deq = codes * h["scale"][None] + h["beta"][None]
        Lq, Lpre = deq + bound, deq
        cq = h["codebooks"][0][i0] + h["codebooks"][1][i1]
        if h["delta"]:
            if prev is None:
                raise ValueError(f"delta frame {k} has no predecessor")
            if n > prev[0].shape[0]:
                raise ValueError(f"delta frame {k} has {n} splats, its predecessor {prev[0].shape[0]}")
            xq, Lq, Lpre, cq = xq + prev[0][:n], Lq + prev[1][:n], Lpre + prev[1][:n], cq + prev[2][:n]
        out.append((xq, Lq, cq, Lpre))
        prev = (xq, Lpre, cq)
    return out


def unpack_frames(streams: Sequence[bytes], device, cholesky_bound=None, prev=None):
    """One gsvc_unpack_splats launch for the concatenated frame streams:
    ``(xq, Lq, cq, Lpre, sizes, (H, W))`` with the frames' splats concatenated.
    ``prev`` = (xq, Lpre, cq) of the frame before the first (device tensors).
    A list that holds entropy-coded frames goes through gsvc_unpack_stream: one
    launch expands every frame to version-1 bytes on the device, then the same
    walk runs on those."""
    device = torch.device(device)
    blob = b"".join(streams)
    offs = [0]
    for s in streams:
        offs.append(offs[-1] + len(s))
    # every header is checked here before anything is sized by it (ValueError);
    # the entry checks them again, and what spans frames, before it launches
    heads = [parse_header(s) for s in streams]
    sizes = [h["N"] for h in heads]
    hw = (heads[0]["H"], heads[0]["W"]) if heads else (0, 0)
    total = sum(sizes)
    if cholesky_bound is None:
        cholesky_bound = torch.tensor([0.5, 0.0, 0.5], device=device)
    bound = cholesky_bound.detach().to(device=device, dtype=torch.float32).contiguous()
    dev_stream = torch.frombuffer(bytearray(blob or b"\0"), dtype=torch.uint8).to(device)
    xq = torch.empty((total, 2), dtype=torch.float32, device=device)
    Lq, cq, Lpre = (torch.empty((total, 3), dtype=torch.float32, device=device) for _ in range(3))
    offs_c = (ctypes.c_longlong * len(offs))(*offs)
    p = [None, None, None]
    prev_n = 0
    if prev is not None:
        p = [t.detach().to(device=device, dtype=torch.float32).contiguous() for t in prev]
        prev_n = p[0].shape[0]
    args = (len(streams), ctypes.c_char_p(blob), offs_c, L.ptr(dev_stream), L.ptr(bound), L.ptr(p[0]),
            L.ptr(p[1]), L.ptr(p[2]), prev_n, L.ptr(xq), L.ptr(Lq), L.ptr(cq), L.ptr(Lpre), total)
    if any(h["version"] == STREAM_VERSION_CODED for h in heads):
        work = torch.empty((HEADER_BYTES * len(streams) + SPLAT_BYTES * total,), dtype=torch.uint8,
                           device=device)
        L.call("gsvc_unpack_stream", *args, L.ptr(work), work.numel(), L.stream(device))
    else:
        L.call("gsvc_unpack_splats", *args, L.stream(device))
    return xq, Lq, cq, Lpre, sizes, (int(hw[0]), int(hw[1]))


def decode_frames(streams: Sequence[bytes], device, prev=None, return_state: bool = False,
                  output: str = "rgb", reference=None, fmt=None, size=None, crop=None, aa=None):
    """Frame streams (``encode_frame``, either version, in any mix) to images
    [F, 3, H, W], or with ``output="i420"`` (or, beside a ``fmt``, its synonym
    ``"yuv"``) to YUV
    frames, uint8 [F, fmt.frame_bytes(H, W)] (``video.rgb_to_i420`` of those
    images in the pixel format ``fmt``, a ``video.YuvFormat`` of any depth,
    chroma and layout; None: planar 8-bit I420, BT.601 limited range; with
    ``reference``, the source's frames in that format, the pair (frames, int64
    [F, 3] squared error)).

    On a HIP device: one unpack launch for all frames, then
    ``render_frames_sum``.  A delta frame adds the DECODED parameters of the
    frame before it; ``prev`` carries them from an earlier call
    (``return_state=True`` also returns (xq, Lpre, cq) of the last frame).
    CPU: the numpy decoder and the CPU operators, frame by frame.

    ``size=(H2, W2)`` and ``crop=(x0, y0, w, h)`` (source pixels, fractions
    allowed) decode through a ``render.View``: the frame models, functions of
    position, sampled at the view's positions -- images [F, 3, H2, W2], and
    ``output="i420"`` / ``fmt`` at H2 x W2.  Unpacking, ``prev`` and the
    returned state are the source's and do not depend on the view.  A view
    that is not the identity cannot take ``reference`` frames (they have the
    source's size): ValueError, as for a window outside the frame, a
    non-positive size or a size the pixel format does not allow.  On the CPU
    the view goes through the CPU statement of the resampled forward.

    ``aa`` (k, (ky, kx) or "auto"; ``render.View``) box-filters the view inside
    the composite, every output pixel the mean of ky x kx point samples: the
    prefilter a downscale needs.  It may be given without ``size`` (a
    supersampled image at the source's size); ``output="i420"`` and ``fmt``
    apply to the filtered images."""
    device = torch.device(device)
    if output not in ("rgb", "i420", "yuv"):
        raise ValueError(f"decode_frames: output is 'rgb', 'i420' or 'yuv', not {output!r}")
    if output == "yuv":  # a synonym: the frames of ``fmt``, whatever its chroma and layout
        if fmt is None:  # without a format it stays the error it was
            raise ValueError("decode_frames: output='yuv' names the frames of a pixel format: pass fmt=")
        output = "i420"
    if reference is not None and output != "i420":
        raise ValueError("decode_frames: reference frames are compared in I420 (output='i420')")
    if fmt is not None and output != "i420":
        raise ValueError("decode_frames: a pixel format applies to output='i420'")
    if len(streams) == 0:
        raise ValueError("decode_frames: no frames")
    view = None
    if size is not None or crop is not None or aa is not None:
        from .render import view_of
        h0 = parse_header(streams[0])
        view = view_of(h0["H"], h0["W"], size, crop, aa)  # ValueError: the window, the size, aa
        if reference is not None and not view.is_identity:
            raise ValueError("decode_frames: reference frames have the source's size; a view that is "
                             "not the identity cannot be compared with them")
        if output == "i420":
            from .video import YuvFormat
            (fmt or YuvFormat()).check_size(view.out_h, view.out_w)
    if device.type == "cuda":
        xq, Lq, cq, Lpre, sizes, (H, W) = unpack_frames(streams, device, prev=prev)
        bg = torch.ones(3, device=device)
        if view is None:
            imgs = render_frames_sum(xq, Lq, cq, sizes, H, W, bg, xyz_tanh=True, cholesky_bound=None)
        else:
            imgs = render_frames_sum(xq, Lq, cq, sizes, H, W, bg, xyz_tanh=True, cholesky_bound=None,
                                     view=view)
        last = sum(sizes[:-1])
        state = (xq[last:], Lpre[last:], cq[last:])
    else:
        p = None if prev is None else tuple(np.asarray(t.detach().cpu().numpy(), np.float32) for t in prev)
        frames = unpack_frames_host(streams, prev=p)
        h0 = parse_header(streams[0])
        H, W = h0["H"], h0["W"]
        tb = ((W + 15) // 16, (H + 15) // 16, 1)
        imgs = []
        for xq, Lq, cq, _ in frames:
            n = xq.shape[0]
            if view is not None:
                from .cpu import render_sum_view
                imgs.append(render_sum_view(torch.tanh(torch.from_numpy(xq)), torch.from_numpy(Lq),
                                            torch.from_numpy(cq), torch.ones(n, 1), torch.ones(3), view))
                continue
            xys, depths, radii, conics, nth = project_gaussians_2d(
                torch.tanh(torch.from_numpy(xq)), torch.from_numpy(Lq), H, W, tb)
            img = rasterize_gaussians_sum(xys, depths, radii, conics, nth, torch.from_numpy(cq),
                                          torch.ones(n, 1), H, W, 16, 16, background=torch.ones(3),
                                          return_alpha=False)
            imgs.append(torch.clamp(img, 0, 1).view(H, W, 3).permute(2, 0, 1))
        imgs = torch.stack(imgs).contiguous()
        xq, _, cq, Lpre = frames[-1]
        state = tuple(torch.from_numpy(np.ascontiguousarray(t)) for t in (xq, Lpre, cq))
    if output == "i420":
        from .video import rgb_to_i420
        imgs = rgb_to_i420(imgs, reference, fmt)
    return (imgs, state) if return_state else imgs


# --------------------------------------------------------------------------
# the video loop

def _load_overfit(model, cur: dict, prev: Optional[dict]) -> None:
    """train_video_Compress.py:51-80: parameters from the overfit checkpoint; a
    delta model gets current - previous, and the PREVIOUS frame's parameters
    in its p_* buffers.  The reference as written stores the CURRENT frame's
    (its :65-71 reads pretrained_dict, the current checkpoint), so its delta
    model starts at 2 current - previous; that is not reproduced here."""
    sd = model.state_dict()
    names = ("_xyz", "_cholesky", "_features_dc")
    for k in names:
        if k not in cur:
            continue
        v = cur[k].to(sd[k].device, torch.float32)
        if prev is not None:
            p = prev[k].to(sd[k].device, torch.float32)[: v.shape[0]]
            sd["p" + k] = p
            v = v - p
        sd[k] = v
    model.load_state_dict(sd)


def compress_video(state_dict: dict, frames: Sequence[torch.Tensor], K_frames: Sequence[int] = (1,),
                   iterations: int = 30000, lr: float = 1e-3, device="cuda:0", loss_type="L2",
                   delta_base: str = "overfit", seed: Optional[int] = None, entropy: bool = False,
                   segment: int = 32, fused: bool = False, run: Optional[int] = None,
                   yuv_loss=None) -> dict:
    """Fine-tune every overfit frame model of ``state_dict`` (``frame_<i>`` ->
    {_xyz, _cholesky, _features_dc}, i from 1) under quantization against
    ``frames`` ([1,3,H,W] each) and encode it: frames listed in ``K_frames``
    (1-based) as key frames, the others as deltas on the frame before.

    ``delta_base="overfit"`` is the reference: a delta is trained against the
    previous frame's UNQUANTIZED overfit parameters
    (train_video_Compress.py:65-71), which a decoder never has, so frames
    decoded in sequence drift from the trained renders by the previous frames'
    quantization error.  ``"decoded"`` trains each delta against
    what the decoder holds -- the previous frame's decoded parameters -- and
    then ``decode_frames`` reproduces the trained eval renders bit for bit.

    Returns {"streams", "psnr", "bpp" (fixed-length), "bpp_entropy_estimate",
    "state_dicts"}; the best-PSNR state of each frame is kept, as the reference
    does.  With ``entropy`` the streams are entropy-coded (version 2, segments
    of ``segment`` splats) and "bpp_coded" gives their ``8 * len / (H * W)``.
    ``fused`` runs every iteration as ``train_iter_quantize_fused`` (one C call;
    HIP devices and the L2 / L1 / YUV losses only -- anything else raises;
    ``loss_type="YUV"`` trains against the weighted Y/U/V loss of ``yuv_loss``,
    a video.YuvLoss, while the best state is still the best RGB PSNR's).  With
    ``run=K`` (``fused`` only) a frame is trained in runs of K iterations, one
    ``train_run_quantize_fused`` call each and a last shorter one, and the best
    state is kept on the device (``QuantBestState``) instead of a host
    comparison and a ``deepcopy`` per iteration: the same streams and states."""
    if delta_base not in ("overfit", "decoded"):
        raise ValueError("delta_base is 'overfit' or 'decoded'")
    if run is not None:
        if not fused:
            raise ValueError("run= needs fused=True")
        if int(run) < 1:
            raise ValueError(f"run = {run}, not >= 1")
    if seed is not None:
        torch.manual_seed(seed)
    device = torch.device(device)
    streams: List[bytes] = []
    psnrs, bpps, bpps_est, bpps_coded, sds = [], [], [], [], {}
    decoded_prev = None
    for i, gt in enumerate(frames):
        num = i + 1
        cur = state_dict[f"frame_{num}"]
        key = num in K_frames or i == 0
        gt = gt.to(device)
        H, W = gt.shape[-2], gt.shape[-1]
        cls = GaussianVideoFrameQ if key else GaussianVideoDelta
        model = cls(loss_type=loss_type, yuv_loss=yuv_loss, opt_type="adan",
                    num_points=cur["_xyz"].shape[0], H=H, W=W,
                    BLOCK_H=16, BLOCK_W=16, device=device, lr=lr, quantize=True).to(device)
        prev = None
        if not key:
            if delta_base == "decoded":
                prev = dict(zip(("_xyz", "_cholesky", "_features_dc"), decoded_prev))
            else:
                prev = state_dict[f"frame_{num - 1}"]
        _load_overfit(model, cur, prev)
        model._init_data()
        model.train()
        if run is not None:
            best, left = QuantBestState(model), int(iterations)
            while left > 0:
                model.train_run_quantize_fused(gt, min(int(run), left), best)
                left -= min(int(run), left)
            best.load_into(model)
        else:
            best_psnr, best_sd = -math.inf, None
            train_iter = model.train_iter_quantize_fused if fused else model.train_iter_quantize
            for _ in range(int(iterations)):
                _, psnr = train_iter(gt)
                if psnr > best_psnr:
                    best_psnr, best_sd = psnr, copy.deepcopy(model.state_dict())
            if best_sd is not None:
                model.load_state_dict(best_sd)
        model.eval()
        with torch.no_grad():
            out = model.forward_quantize()
            mse = F.mse_loss(out["render"].float(), gt.float()).item()
        psnrs.append(10 * math.log10(1.0 / mse) if mse > 0 else math.inf)
        bpps.append(sum(b.fixed for b in out["unit_bit"]) / H / W)
        bpps_est.append(sum(b.entropy_estimate for b in out["unit_bit"]) / H / W)
        streams.append(encode_frame(model, entropy=entropy, segment=segment))
        bpps_coded.append(8 * len(streams[-1]) / H / W)
        sds[f"frame_{num}"] = {k: v for k, v in model.state_dict().items()
                               if k in ("_xyz", "_cholesky", "_features_dc")}
        if delta_base == "decoded":
            dprev = None if key else decoded_prev
            if device.type == "cuda":
                xq, _, cq, Lpre, _, _ = unpack_frames([streams[-1]], device,
                                                      model.cholesky_bound, prev=dprev)
                decoded_prev = (xq, Lpre, cq)
            else:
                p = None if dprev is None else tuple(t.cpu().numpy() for t in dprev)
                xq, _, cq, Lpre = unpack_frames_host([streams[-1]], prev=p)[0]
                decoded_prev = tuple(torch.from_numpy(np.ascontiguousarray(t)) for t in (xq, Lpre, cq))
    out = {"streams": streams, "psnr": psnrs, "bpp": bpps, "bpp_entropy_estimate": bpps_est,
           "state_dicts": sds}
    if entropy:
        out["bpp_coded"] = bpps_coded
    return out


__all__ = ["GaussianVideoFrameQ", "GaussianVideoDelta", "QuantBestState", "Bits", "encode_frame", "encode_frames",
           "decode_frames",
           "unpack_frames", "unpack_frames_host", "pack_planes_host", "parse_header",
           "compress_video", "HEADER_BYTES", "SPLAT_BYTES", "STREAM_MAGIC", "STREAM_VERSION",
           "STREAM_VERSION_CODED", "entropy_code", "entropy_expand"]
