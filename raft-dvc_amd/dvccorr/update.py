"""The update block's GRU on the MI355X: SepConvGRU3D.forward (src/core/update.py:139-199) as three fused launches.

    gru = dvccorr.SepConvGRU(update_block.gru.state_dict())      # once per weight set
    net = gru(net, inp)                                          # update.py:341, net = self.gru(net, inp)

Per axis a in (h, w, d), with conv_*_a a 5-tap 1-D convolution zero-padded by 2 along a:

    hx = cat[h, x];  z = sigmoid(convz_a(hx));  r = sigmoid(convr_a(hx))
    q  = tanh(convq_a(cat[r * h, x]));  h = (1 - z) * h + z * q

k_sep_gru_pass (csrc/gru.hip) runs one pass per launch on the matrix cores; z, r, q and hx never reach memory.
Precision follows resolve_precision: "fp16" / "bf16" (also inside a CUDA autocast region, the reference under its
Trainer's AMP) round the operands once and accumulate in fp32; "fp32" splits them into bf16 hi + lo pieces (fp32
tolerance 1e-5).  The gates, the blend and the returned hidden state are float32 in every precision.

Forward only: inputs or weights that require grad (with grad enabled) raise NotImplementedError.  The kernel covers
hidden 96 and input <= 160 (the reference model: 96 and 147); other channel counts run the same composition as
F.conv3d calls on the GPU.
"""
from __future__ import annotations

from typing import Mapping, Optional

import torch
import torch.nn.functional as F

from . import _lib, ops
from .corr_block import _wants_grad, resolve_precision

__all__ = ["SepConvGRU", "sep_conv_gru", "GRU_WEIGHT_NAMES"]

_AXES = (("h", (2, 0, 0)), ("w", (0, 2, 0)), ("d", (0, 0, 2)))
GRU_WEIGHT_NAMES = tuple(f"conv{g}_{ax}.{kind}" for ax, _ in _AXES for g in "zrq" for kind in ("weight", "bias"))


def _validate(h: torch.Tensor, x: torch.Tensor, weights: Mapping[str, torch.Tensor]) -> None:
    if h.ndim != 5 or x.ndim != 5:
        raise ValueError(f"sep_conv_gru: h and x must be (B, C, H, W, D); got h {tuple(h.shape)} x {tuple(x.shape)}")
    if h.shape[0] != x.shape[0] or h.shape[2:] != x.shape[2:]:
        raise ValueError(f"sep_conv_gru: batch / spatial sizes differ: h {tuple(h.shape)} x {tuple(x.shape)}")
    missing = [n for n in GRU_WEIGHT_NAMES if n not in weights]
    if missing:
        raise ValueError(f"sep_conv_gru: missing weights {missing} (SepConvGRU3D.state_dict() names)")
    hidden, cin = h.shape[1], h.shape[1] + x.shape[1]
    for ax, _ in _AXES:
        for g in "zrq":
            w, b = weights[f"conv{g}_{ax}.weight"], weights[f"conv{g}_{ax}.bias"]
            if w.ndim != 5 or w.shape[0] != hidden or w.shape[1] != cin or w.numel() != hidden * cin * 5 \
                    or w.shape[2 + "hwd".index(ax)] != 5 or tuple(b.shape) != (hidden,):
                raise ValueError(f"sep_conv_gru: conv{g}_{ax} weight {tuple(w.shape)} bias {tuple(b.shape)} do not "
                                 f"match hidden {hidden} + input {x.shape[1]} channels (h {tuple(h.shape)} "
                                 f"x {tuple(x.shape)})")


def _refuse_grad(h, x, weights) -> None:
    if _wants_grad(h, x, *(weights[n] for n in GRU_WEIGHT_NAMES)):
        raise NotImplementedError("dvccorr.sep_conv_gru has no backward; call it under torch.no_grad() or use the "
                                  "reference's SepConvGRU3D for gradients")


def kernel_covers(hidden: int, inp: int) -> bool:
    return hidden == _lib.GRU_HIDDEN and 1 <= inp <= _lib.GRU_MAX_INPUT


def _composition(h: torch.Tensor, x: torch.Tensor, weights: Mapping[str, torch.Tensor]) -> torch.Tensor:
    """The reference's nine convolutions in float32, for channel counts outside the kernel's."""
    p = {n: weights[n].detach().float() for n in GRU_WEIGHT_NAMES}
    h, x = h.detach().float(), x.detach().float()
    with torch.autocast("cuda", enabled=False):
        for ax, pad in _AXES:
            hx = torch.cat([h, x], dim=1)
            z = torch.sigmoid(F.conv3d(hx, p[f"convz_{ax}.weight"], p[f"convz_{ax}.bias"], padding=pad))
            r = torch.sigmoid(F.conv3d(hx, p[f"convr_{ax}.weight"], p[f"convr_{ax}.bias"], padding=pad))
            q = torch.tanh(F.conv3d(torch.cat([r * h, x], dim=1), p[f"convq_{ax}.weight"], p[f"convq_{ax}.bias"],
                                    padding=pad))
            h = (1 - z) * h + z * q
    return h


def _run(h, x, weights, precision, packed_fn) -> torch.Tensor:
    _validate(h, x, weights)
    ops._need_cuda(h, x, *(weights[n] for n in GRU_WEIGHT_NAMES))
    _refuse_grad(h, x, weights)
    if not kernel_covers(h.shape[1], x.shape[1]):
        return _composition(h, x, weights)
    dtype = ops.dtype_code(resolve_precision(h, precision))
    return torch.ops.dvccorr.sep_gru(h.detach(), x.detach(), packed_fn(dtype), dtype)


def sep_conv_gru(h: torch.Tensor, x: torch.Tensor, weights: Mapping[str, torch.Tensor], *,
                 precision: Optional[str] = None) -> torch.Tensor:
    """SepConvGRU3D.forward(h, x) with the module's state_dict() `weights`; returns the new hidden state (float32).
    Packs the weights on every call: keep a SepConvGRU where the same weights serve many calls."""
    return _run(h, x, weights, precision, lambda dtype: ops.gru_pack(weights, dtype))


class SepConvGRU:
    """sep_conv_gru with the packed weights cached per precision.  An entry belongs to the eighteen tensor objects,
    their in-place version counters and their storage, so an optimiser step or load_state_dict (in-place updates) and
    a replaced tensor all re-pack."""

    def __init__(self, weights: Mapping[str, torch.Tensor], precision: Optional[str] = None):
        missing = [n for n in GRU_WEIGHT_NAMES if n not in weights]
        if missing:
            raise ValueError(f"SepConvGRU: missing weights {missing} (SepConvGRU3D.state_dict() names)")
        self.weights = weights
        self.precision = precision
        self._packed: dict = {}

    def _state(self):
        ts = [self.weights[n] for n in GRU_WEIGHT_NAMES]
        return tuple((id(t), t._version, t.data_ptr(), tuple(t.shape), t.device) for t in ts)

    def packed(self, dtype: int) -> torch.Tensor:
        state = self._state()
        hit = self._packed.get(dtype)
        if hit is None or hit[0] != state:
            # the tensors are kept alive beside the entry, so their ids cannot be reused while it is valid
            hit = (state, ops.gru_pack(self.weights, dtype), [self.weights[n] for n in GRU_WEIGHT_NAMES])
            self._packed[dtype] = hit
        return hit[1]

    def __call__(self, h: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        return _run(h, x, self.weights, self.precision, self.packed)
