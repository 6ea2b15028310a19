"""Quantizers of the compression stage (GSVC's quantize.py, restated).

``FakeQuantizationHalf`` and ``UniformQuantizer`` follow quantize.py:15-87: the
same constructor arguments, the ``scale`` / ``beta`` parameter names (so the
reference's state-dict keys load), ``_init_data``, ``compress`` and
``decompress``.  ``ResidualVQ8`` stands in for the reference's
``vector_quantize_pytorch.ResidualVQ(dim=3, codebook_size=8, num_quantizers=2,
decay=0.8, commitment_weight=1., kmeans_init=True, kmeans_iters=5)``: that
package is not a dependency here, so the semantics below are this project's
own statement of the documented algorithm and parity with the package is
unpinned.

``quantize_params`` is the hot path: one autograd Function over the gfx950
kernels of csrc/quant.hip (gsvc_quant_params_forward / _backward) for CUDA
tensors; CPU tensors take the same op sequence in torch ops.  Nothing falls
back: a CUDA call without the library raises.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor, nn

from . import _lib as L

QMAX6 = 63
CODEWORDS = 8
STAGES = 2


class FakeQuantizationHalf(torch.autograd.Function):
    """x -> float(half(x)), identity gradient (quantize.py:15-24)."""

    @staticmethod
    def forward(_, x):
        return x.half().float()

    @staticmethod
    def backward(_, grad_output):
        return grad_output


def zeroth_order_bits(symbols) -> Tuple[float, int]:
    """(sum_i -n_i log2(n_i / N), number of distinct symbols) of an integer
    array: the zeroth-order entropy of the codes, an ESTIMATE of what the
    reference's ANS coder (constriction, not available here) would write."""
    a = np.asarray(symbols).reshape(-1)
    if a.size == 0:
        return 0.0, 0
    counts = np.bincount(a.astype(np.int64))
    counts = counts[counts > 0].astype(np.float64)
    return float(-(counts * np.log2(counts / a.size)).sum()), int(counts.size)


def _table_bits(unique: int) -> int:
    # quantize.py:74-77: the histogram (int64 counts) and the symbol list (uint8)
    return unique * (64 + 8)


class UniformQuantizer(nn.Module):
    def __init__(self, signed=False, bits=8, learned=False, num_channels=1, entropy_type="none",
                 weight=0.001):
        super().__init__()
        if signed:
            self.qmin, self.qmax = -2 ** (bits - 1), 2 ** (bits - 1) - 1
        else:
            self.qmin, self.qmax = 0, 2 ** bits - 1
        self.learned = learned
        self.entropy_type = entropy_type
        if learned:
            self.scale = nn.Parameter(torch.ones(num_channels) / self.qmax)
            self.beta = nn.Parameter(torch.ones(num_channels) / self.qmax)
        self.weight = weight

    def _init_data(self, tensor):
        t_min, t_max = tensor.min(dim=0)[0], tensor.max(dim=0)[0]
        self.beta.data = t_min.detach().clone()
        self.scale.data = ((t_max - t_min) / (self.qmax - self.qmin)).detach()

    def forward(self, x):
        """(dequantized, entropy loss (0), bits): the general torch-op path for
        any bit width (quantize.py:51-70).  The frame models call
        ``quantize_params`` instead, which has this arithmetic for 6 bits."""
        if self.learned:
            code = ((x - self.beta) / self.scale).clamp(self.qmin, self.qmax)
            quant = (code.round() - code).detach() + code
            dequant = quant * self.scale + self.beta
        else:
            code = (x * self.qmax).clamp(self.qmin, self.qmax)
            quant = (code.round() - code).detach() + code
            dequant = quant / self.qmax
        bits = 0 if self.training else self.size(quant)
        return dequant, 0 * self.weight, bits

    def size(self, quant):
        """Estimated bits of the codes: zeroth-order entropy + the tables
        quantize.py:72-80 counts (histogram, symbols, scale, beta)."""
        h, unique = zeroth_order_bits(quant.detach().round().to(torch.int64).cpu().numpy()
                                      - self.qmin)
        bits = h + _table_bits(unique)
        if self.learned:
            bits += (self.scale.numel() + self.beta.numel()) * 32
        return bits

    def compress(self, x):
        code = ((x - self.beta) / self.scale).clamp(self.qmin, self.qmax).round()
        return code, code * self.scale + self.beta

    def decompress(self, x):
        return x * self.scale + self.beta


def _nearest(r: Tensor, cb: Tensor) -> Tuple[Tensor, Tensor]:
    """Nearest codeword of cb [K,3] to each row of r [N,3]: (index, squared
    distance), the distance summed over d ascending and the lowest index of
    equal distances (the kernel's rule; torch.argmin does not promise one)."""
    diff = r[:, None, :] - cb[None, :, :]
    sq = diff * diff
    d = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
    dmin = d.min(dim=1).values
    ids = torch.arange(cb.shape[0], device=r.device).expand_as(d)
    idx = torch.where(d == dmin[:, None], ids, torch.full_like(ids, cb.shape[0])).min(dim=1).values
    return idx.clamp_(max=cb.shape[0] - 1), dmin


def _cluster_sums(r: Tensor, idx: Tensor, k: int) -> Tuple[Tensor, Tensor]:
    """(members per codeword [k], sum of members [k,3]) by masked reductions:
    no atomics, so equal inputs give equal bits."""
    onehot = (idx[:, None] == torch.arange(k, device=r.device)[None, :]).to(r.dtype)
    return onehot.sum(0), (onehot[:, :, None] * r[:, None, :]).sum(0)


class ResidualVQ8(nn.Module):
    """Two-stage residual vector quantizer, 8 codewords x 3 dims per stage.

    Stage 0 quantizes f, stage 1 the residual f - e0; the output is e0 + e1.
    Codebooks start from k-means (5 iterations, seeded from torch's global
    generator) on first use and follow an exponential moving average (decay
    0.8) of their members in training mode.  Each stage is straight-through on
    its own residual, so d(e0 + e1)/df = 2 I (the second stage's residual
    subtracts a detached e0); the commitment loss per stage is
    mean((r_i - e_i)^2) with weight 1.
    """

    def __init__(self, decay: float = 0.8, kmeans_iters: int = 5, eps: float = 1e-5,
                 commitment_weight: float = 1.0):
        super().__init__()
        self.decay, self.kmeans_iters, self.eps = decay, kmeans_iters, eps
        self.commitment_weight = commitment_weight
        self.register_buffer("codebooks", torch.zeros(STAGES, CODEWORDS, 3))
        self.register_buffer("cluster_size", torch.zeros(STAGES, CODEWORDS))
        self.register_buffer("embed_avg", torch.zeros(STAGES, CODEWORDS, 3))
        self.register_buffer("initted", torch.zeros((), dtype=torch.bool))
        self._initted_host = None  # the buffer's value once read (no device sync per step)

    def is_initted(self) -> bool:
        if self._initted_host is None:
            self._initted_host = bool(self.initted)
        return self._initted_host

    def _load_from_state_dict(self, *args, **kwargs):
        self._initted_host = None
        return super()._load_from_state_dict(*args, **kwargs)

    @torch.no_grad()
    def init_codebooks(self, x: Tensor) -> None:
        r = x.detach().float()
        n = r.shape[0]
        for s in range(STAGES):
            if n >= CODEWORDS:
                pick = torch.randperm(n)[:CODEWORDS]
            else:
                pick = torch.randint(0, max(n, 1), (CODEWORDS,))
            means = r[pick.to(r.device)].clone() if n > 0 else torch.zeros(CODEWORDS, 3, device=r.device)
            counts = torch.zeros(CODEWORDS, device=r.device)
            for _ in range(self.kmeans_iters if n > 0 else 0):
                idx, _ = _nearest(r, means)
                counts, sums = _cluster_sums(r, idx, CODEWORDS)
                means = torch.where(counts[:, None] > 0, sums / counts.clamp(min=1)[:, None], means)
            self.codebooks[s] = means
            self.cluster_size[s] = counts
            self.embed_avg[s] = means * counts[:, None]
            if n > 0:
                idx, _ = _nearest(r, means)
                r = r - means[idx]
        self.initted.fill_(True)
        self._initted_host = True

    @torch.no_grad()
    def ema_update(self, x: Tensor, codes_rgb: Tensor) -> None:
        """Move the codebooks towards their members: ``codes_rgb`` [N,2] are the
        indices the quantizer returned for ``x`` with the current codebooks."""
        r = x.detach().float()
        idx = codes_rgb.long()
        old = self.codebooks.clone()
        for s in range(STAGES):
            counts, sums = _cluster_sums(r, idx[:, s], CODEWORDS)
            self.cluster_size[s].mul_(self.decay).add_(counts, alpha=1 - self.decay)
            self.embed_avg[s].mul_(self.decay).add_(sums, alpha=1 - self.decay)
            total = self.cluster_size[s].sum()
            smoothed = (self.cluster_size[s] + self.eps) / (total + CODEWORDS * self.eps) * total
            self.codebooks[s] = self.embed_avg[s] / smoothed[:, None]
            r = r - old[s][idx[:, s]]

    def forward(self, x: Tensor):
        """(quantized, indices [N,2], commitment loss per stage [2]) by
        ``quantize_params``' colour path alone."""
        if not self.is_initted():
            self.init_codebooks(x)
        cq, codes, sums = _vq_only(x, self.codebooks)
        if self.training:
            self.ema_update(x, codes)
        return cq, codes, sums / max(x.numel(), 1) * self.commitment_weight

    def decompress(self, codes_rgb: Tensor) -> Tensor:
        idx = codes_rgb.long()
        return self.codebooks[0][idx[:, 0]] + self.codebooks[1][idx[:, 1]]


# --------------------------------------------------------------------------
# quantize_params: the op sequence of csrc/quant.hip

def _forward_torch(xyz, chol, feat, scale, beta, cb, bound, prev, commit):
    xq = xyz.half().float()
    raw = (chol - beta) / scale
    # the kernel's fmaxf(raw, 0) drops a NaN: code 0 and a finite Lq
    q = torch.where(raw != raw, torch.zeros_like(raw), raw).clamp(0, QMAX6).round()
    Lq = (q * scale + beta) + bound.reshape(1, 3)
    i0, d0 = _nearest(feat, cb[0])
    e0 = cb[0][i0]
    i1, d1 = _nearest(feat - e0, cb[1])
    cq = e0 + cb[1][i1]
    if prev is not None:
        xq, Lq, cq = xq + prev[0], Lq + prev[1], cq + prev[2]
    codes_chol = q.to(torch.uint8)
    codes_rgb = torch.stack([i0, i1], dim=1).to(torch.uint8)
    sums = torch.stack([d0.sum(), d1.sum()]) if commit else None
    return xq, Lq, cq, codes_chol, codes_rgb, sums


def _backward_torch(chol, feat, scale, beta, cb, codes_rgb, v_xq, v_Lq, v_cq, v_commit):
    raw = (chol - beta) / scale
    q = torch.where(raw != raw, torch.zeros_like(raw), raw).clamp(0, QMAX6).round()
    mask = ((raw >= 0) & (raw <= QMAX6)).to(raw.dtype)
    v_chol = v_Lq * mask
    v_scale = (v_Lq * (q - mask * raw)).sum(0)
    v_beta = (v_Lq * (1 - mask)).sum(0)
    v_feat = 2 * v_cq
    if v_commit is not None:
        idx = codes_rgb.long()
        r1 = feat - cb[0][idx[:, 0]]
        v_feat = v_feat + (v_commit[0] * (2 * r1) + v_commit[1] * (2 * (r1 - cb[1][idx[:, 1]])))
    return v_xq.clone(), v_chol, v_feat, v_scale, v_beta


def _f32c(t: Tensor) -> Tensor:
    t = t.detach()
    if t.dtype is not torch.float32 or not t.is_contiguous():
        t = t.float().contiguous()
    return t


def _workspace(n: int, dev) -> Tensor:
    return torch.empty((L.size("gsvc_quant_workspace_bytes", n),), dtype=torch.uint8, device=dev)


def _forward_hip(xyz, chol, feat, scale, beta, cb, bound, prev, commit):
    n, dev = xyz.shape[0], xyz.device
    xq, Lq, cq = torch.empty_like(xyz), torch.empty_like(chol), torch.empty_like(feat)
    codes_chol = torch.empty((n, 3), dtype=torch.uint8, device=dev)
    codes_rgb = torch.empty((n, 2), dtype=torch.uint8, device=dev)
    # without the sums the kernel skips its reduction and the combine launch
    sums = torch.empty((2,), dtype=torch.float32, device=dev) if commit else None
    ws = _workspace(n, dev) if commit else None
    p = prev if prev is not None else (None, None, None)
    L.call("gsvc_quant_params_forward", n, L.ptr(xyz), L.ptr(chol), L.ptr(feat), L.ptr(scale),
           L.ptr(beta), L.ptr(cb), L.ptr(bound), L.ptr(p[0]), L.ptr(p[1]), L.ptr(p[2]), L.ptr(xq),
           L.ptr(Lq), L.ptr(cq), L.ptr(codes_chol), L.ptr(codes_rgb), L.ptr(sums), L.ptr(ws),
           ws.numel() if commit else 0, L.stream(dev))
    return xq, Lq, cq, codes_chol, codes_rgb, sums


def _backward_hip(chol, feat, scale, beta, cb, codes_rgb, v_xq, v_Lq, v_cq, v_commit):
    n, dev = chol.shape[0], chol.device
    v_xyz = torch.empty((n, 2), dtype=torch.float32, device=dev)
    v_chol, v_feat = torch.empty_like(chol), torch.empty_like(feat)
    v_scale = torch.empty((3,), dtype=torch.float32, device=dev)
    v_beta = torch.empty((3,), dtype=torch.float32, device=dev)
    ws = _workspace(n, dev)
    L.call("gsvc_quant_params_backward", n, L.ptr(chol), L.ptr(feat), L.ptr(scale), L.ptr(beta),
           L.ptr(cb), L.ptr(codes_rgb), L.ptr(v_xq), L.ptr(v_Lq), L.ptr(v_cq), L.ptr(v_commit),
           L.ptr(v_xyz), L.ptr(v_chol), L.ptr(v_feat), L.ptr(v_scale), L.ptr(v_beta), L.ptr(ws),
           ws.numel(), L.stream(dev))
    return v_xyz, v_chol, v_feat, v_scale, v_beta


def _check(xyz, chol, feat, scale, beta, cb, bound, prev):
    n = xyz.shape[0]
    if xyz.shape != (n, 2) or chol.shape != (n, 3) or feat.shape != (n, 3):
        raise ValueError("quantize_params: xyz [N,2], cholesky [N,3], features [N,3] expected")
    if scale.numel() != 3 or beta.numel() != 3 or bound.numel() != 3:
        raise ValueError("quantize_params: scale, beta and cholesky_bound have 3 elements")
    if tuple(cb.shape) != (STAGES, CODEWORDS, 3):
        raise ValueError("quantize_params: codebooks [2,8,3] expected")
    if prev is not None and (len(prev) != 3 or prev[0].shape != xyz.shape
                             or prev[1].shape != chol.shape or prev[2].shape != feat.shape):
        raise ValueError("quantize_params: prev = (p_xyz [N,2], p_cholesky [N,3], p_features [N,3])")
    devs = {t.device for t in (xyz, chol, feat, scale, beta, cb, bound) + tuple(prev or ())}
    if len(devs) != 1:
        raise RuntimeError(f"quantize_params: tensors on different devices: {sorted(map(str, devs))}")


class _QuantizeParams(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, chol, feat, scale, beta, cb, bound, p_xyz, p_chol, p_feat, commit):
        prev = None if p_xyz is None else tuple(_f32c(t) for t in (p_xyz, p_chol, p_feat))
        args = tuple(_f32c(t) for t in (xyz, chol, feat, scale, beta, cb, bound))
        fwd = _forward_hip if xyz.is_cuda else _forward_torch
        xq, Lq, cq, codes_chol, codes_rgb, sums = fwd(*args, prev, commit)
        # the codebooks move (EMA) between this forward and its backward
        ctx.save_for_backward(args[1], args[2], args[3], args[4], args[5].clone(), codes_rgb)
        ctx.mark_non_differentiable(codes_chol, codes_rgb)
        return xq, Lq, cq, codes_chol, codes_rgb, sums

    @staticmethod
    def backward(ctx, v_xq, v_Lq, v_cq, _cc, _cr, v_sums):
        chol, feat, scale, beta, cb, codes_rgb = ctx.saved_tensors
        bwd = _backward_hip if chol.is_cuda else _backward_torch
        v_xyz, v_chol, v_feat, v_scale, v_beta = bwd(
            chol, feat, scale, beta, cb, codes_rgb, _f32c(v_xq), _f32c(v_Lq), _f32c(v_cq),
            None if v_sums is None else _f32c(v_sums))
        return v_xyz, v_chol, v_feat, v_scale, v_beta, None, None, None, None, None, None


def quantize_params(xyz: Tensor, cholesky: Tensor, features: Tensor, scale: Tensor, beta: Tensor,
                    codebooks: Tensor, cholesky_bound: Tensor,
                    prev: Optional[Tuple[Tensor, Tensor, Tensor]] = None, commit: bool = True):
    """Quantized parameters of a frame model (csrc/quant.hip's op sequence).

    Returns ``(xq, Lq, cq, codes_chol, codes_rgb, commit_sums)``: positions
    through fp16 (before tanh), Cholesky entries through the 6-bit quantizer
    plus ``cholesky_bound``, colours through the residual VQ -- each plus
    ``prev``'s entry for a delta frame --, the uint8 codes, and per VQ stage
    the sum of squared distances to the chosen codeword.  Gradients flow to
    xyz, cholesky, features, scale and beta (straight-through; the codebooks
    follow ``ResidualVQ8.ema_update``, not a gradient).  ``commit=False``
    (inference, encoding) leaves the sums out: ``commit_sums`` is None and the
    kernel runs without its reduction.
    """
    _check(xyz, cholesky, features, scale, beta, codebooks, cholesky_bound, prev)
    p = prev if prev is not None else (None, None, None)
    return _QuantizeParams.apply(xyz, cholesky, features, scale, beta, codebooks, cholesky_bound,
                                 *p, commit)


def _vq_only(x: Tensor, cb: Tensor):
    n = x.shape[0]
    z2, z3 = x.new_zeros(n, 2), x.new_zeros(n, 3)
    one, zero = x.new_ones(3), x.new_zeros(3)
    _, _, cq, _, codes_rgb, sums = quantize_params(z2, z3, x, one, zero, cb, zero)
    return cq, codes_rgb, sums


def vq_loss_from_sums(commit_sums: Tensor, num_points: int, weight: float = 1.0) -> Tensor:
    """Sum over the stages of mean((r_i - e_i)^2) * weight."""
    return commit_sums.sum() * (weight / max(3 * num_points, 1))


def fixed_bits(num_points: int):
    """Bits the packed stream spends per group (positions, Cholesky codes,
    colour indices) on the splats themselves."""
    return 16 * 2 * num_points, 18 * num_points, 6 * num_points


__all__ = ["FakeQuantizationHalf", "UniformQuantizer", "ResidualVQ8", "quantize_params",
           "vq_loss_from_sums", "zeroth_order_bits", "fixed_bits", "QMAX6", "CODEWORDS", "STAGES"]
