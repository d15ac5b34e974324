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

sep_conv_gru and SepConvGRU are forward only: inputs or weights that require grad (with grad enabled) raise
NotImplementedError.  sep_conv_gru_ad is the same GRU with a backward (csrc/gru_grad.hip: the gradients of h, x and
the eighteen parameters) for training.  The kernels cover hidden 96 and input <= 160 (the reference model: 96 and
147); other channel counts run the same composition as F.conv3d calls on the GPU.

The whole of BasicUpdateBlock.forward (update.py:316-348): the motion encoder's convf1 / convf2 / conv and the flow
and uncertainty heads run on k_conv7_flow / k_conv3_mfma (csrc/conv3.hip), with no library convolution and no
torch.cat per iteration:

    block = dvccorr.UpdateBlock(update_block.state_dict())       # once per weight set
    cor = corr_fn.lookup_convc1(coords1, convc1.weight, convc1.bias)
    net, delta_flow, log_b = block(net, context, flow, cor=cor)  # raft_dvc.py:468

conv3x3x3 is the functional form of one such layer, forward only; conv3x3x3_ad is the same layer with a backward
(input, weight and bias gradients on csrc/conv3_grad.hip) for training, conv7x7x7_flow_ad is encoder.convf1 with its
weight and bias gradients (csrc/conv7_grad.hip), and update_block_ad is the whole block as one differentiable call:

    cor = corr_fn.lookup_convc1(coords1, convc1.weight, convc1.bias)         # differentiable (lookup_convc1_ad)
    net, delta_flow, log_b = dvccorr.update_block_ad(net, context, flow, update_block.state_dict(keep_vars=True),
                                                     cor=cor)
"""
from __future__ import annotations

from typing import Mapping, Optional

import torch
import torch.nn.functional as F

from . import _lib, ops
from .corr_block import _wants_grad, resolve_precision

__all__ = ["SepConvGRU", "sep_conv_gru", "sep_conv_gru_ad", "GRU_WEIGHT_NAMES", "UpdateBlock", "conv3x3x3", "conv3x3x3_ad",
           "conv7x7x7_flow_ad", "update_block_ad"]

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


def _refuse_grad(h, x, weights, names=GRU_WEIGHT_NAMES, what="sep_conv_gru", ref="SepConvGRU3D", more=()) -> None:
    if _wants_grad(h, x, *more, *(weights[n] for n in names)):
        hint = {"sep_conv_gru": "dvccorr.sep_conv_gru_ad", "UpdateBlock": "dvccorr.update_block_ad"}.get(
            what, f"the reference's {ref}")
        raise NotImplementedError(f"dvccorr.{what} has no backward; call it under torch.no_grad() or use {hint} "
                                  "for gradients")


class _PackCache:
    """Packed weights per key (a precision, or a layer and a precision).  An entry belongs to the tensor objects it
    was packed from, their in-place version counters and their storage, so an optimiser step or load_state_dict
    (in-place updates) and a replaced tensor all re-pack."""

    def __init__(self):
        self._entries: dict = {}

    @staticmethod
    def state(tensors):
        return tuple((id(t), t._version, t.data_ptr(), tuple(t.shape), t.device) for t in tensors)

    def get(self, key, tensors, pack):
        tensors = list(tensors)
        state = self.state(tensors)
        hit = self._entries.get(key)
        if hit is None or hit[0] != state:
            # the tensors are kept alive beside the entry, so their ids cannot be reused while it is valid
            hit = (state, pack(), tensors)
            self._entries[key] = hit
        return hit[1]


def kernel_covers(hidden: int, inp: int) -> bool:
    return hidden == _lib.GRU_HIDDEN and 1 <= inp <= _lib.GRU_MAX_INPUT


def _composition(h: torch.Tensor, x: torch.Tensor, weights: Mapping[str, torch.Tensor], detach: bool = True) -> torch.Tensor:
    """The reference's nine convolutions in float32, for channel counts outside the kernel's (detach = False: with
    autograd on, for sep_conv_gru_ad)."""
    cut = (lambda t: t.detach().float()) if detach else (lambda t: t.float())
    p = {n: cut(weights[n]) for n in GRU_WEIGHT_NAMES}
    h, x = cut(h), cut(x)
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


def sep_conv_gru_ad(h: torch.Tensor, x: torch.Tensor, weights: Mapping[str, torch.Tensor], *,
                    precision: Optional[str] = None) -> torch.Tensor:
    """sep_conv_gru as a differentiable function: SepConvGRU3D.forward(h, x), float32 out, bit-identical to
    sep_conv_gru's, with gradients for h, x and the eighteen parameters (dvccorr::sep_gru_ad).  The training forward
    (k_sep_gru_pass with SAVE) keeps z, r and q of the three passes and the two intermediate hidden states for the
    backward: 11 x 96 x B H W D floats, 138 MB at 32^3.  The backward runs, per pass in reverse, k_gru_grad_prep,
    k_sep_gru_dgrad (two launches) and k_gru_wgrad, skipping what no input asks for.  Precision as sep_conv_gru, in
    both directions: "fp16" / "bf16" round both operands of every product once and accumulate in fp32, "fp32" splits
    them into bf16 hi + lo pieces.  Under "fp16" the gate gradients are operands and are rounded to fp16 too, as the
    reference's AMP backward does: scale the loss (GradScaler) so that they stay in fp16's range.  The packed weights
    are cached per weight object until it changes (an optimiser step re-packs).  No double backward.  Channel counts
    outside the kernels' (hidden 96, input <= 160) run the float32 composition with autograd on."""
    _validate(h, x, weights)
    ws = [weights[n] for n in GRU_WEIGHT_NAMES]
    ops._need_cuda(h, x, *ws)
    if not kernel_covers(h.shape[1], x.shape[1]):
        return _composition(h, x, weights, detach=False)
    dtype = ops.dtype_code(resolve_precision(h, precision))
    return torch.ops.dvccorr.sep_gru_ad(h, x, ws, dtype)[0]


class SepConvGRU:
    """sep_conv_gru with the packed weights cached per precision (_PackCache: an optimiser step, load_state_dict and
    a replaced tensor all re-pack)."""

    def __init__(self, weights: Mapping[str, torch.Tensor], precision: Optional[str] = None):
        missing = [n for n in GRU_WEIGHT_NAMES if n not in weights]
        if missing:
            raise ValueError(f"SepConvGRU: missing weights {missing} (SepConvGRU3D.state_dict() names)")
        self.weights = weights
        self.precision = precision
        self._packed = _PackCache()

    def packed(self, dtype: int) -> torch.Tensor:
        return self._packed.get(dtype, (self.weights[n] for n in GRU_WEIGHT_NAMES),
                                lambda: ops.gru_pack(self.weights, dtype))

    def __call__(self, h: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        return _run(h, x, self.weights, self.precision, self.packed)


# ---------------------------------------------------------------------------------------------------------------
# BasicUpdateBlock.forward (update.py:316-348)
# ---------------------------------------------------------------------------------------------------------------
_ENCODER_LAYERS = ("encoder.convc1", "encoder.convf1", "encoder.convf2", "encoder.conv")
_HEAD_LAYERS = ("flow_head.conv1", "flow_head.conv2")
_UNC_LAYERS = ("uncertainty_head.conv1", "uncertainty_head.conv2")
_CONVGRU_LAYERS = ("gru.convz", "gru.convr", "gru.convq")


def _wb(layers):
    return tuple(f"{l}.{k}" for l in layers for k in ("weight", "bias"))


def conv_covers(cin: int, cout: int) -> bool:
    """Channel counts k_conv3_mfma runs (dvc_conv3)."""
    return 1 <= cin <= _lib.CONV3_MAX_CIN and 1 <= cout <= _lib.CONV3_MAX_COUT


def _library_conv(x, weight, bias, relu):
    """A layer outside the kernels' shapes: F.conv3d in float32, 'same' padding."""
    with torch.autocast("cuda", enabled=False):
        y = F.conv3d(x.detach().float(), weight.detach().float(), bias.detach().float(),
                     padding=tuple(k // 2 for k in weight.shape[2:]))
        return F.relu(y) if relu else y


def _conv3_layer(cache, key, dtype, src0, src1, weight, bias, dst, offset, relu) -> None:
    """dst[:, offset:offset + cout] = conv(cat[src0, src1]) + bias (+ ReLU): the kernel where it covers the layer."""
    cout, cin = int(weight.shape[0]), int(weight.shape[1])
    if tuple(weight.shape[2:]) == (3, 3, 3) and conv_covers(cin, cout):
        pack = lambda: ops.conv3_pack(weight, bias, dtype)   # noqa: E731
        packed = pack() if cache is None else cache.get((key, dtype), (weight, bias), pack)
        torch.ops.dvccorr.conv3(src0, src1, packed, dst, offset, cout, relu, dtype)
    else:
        x = src0 if src1 is None else torch.cat([src0, src1], dim=1)
        dst[:, offset:offset + cout].copy_(_library_conv(x, weight, bias, relu))


def _same_volume(what, first, *rest) -> None:
    for name, t in (first,) + rest:
        if t.ndim != 5:
            raise ValueError(f"{what}: {name} must be (B, C, H, W, D), got {tuple(t.shape)}")
    (n0, t0) = first
    for name, t in rest:
        if t.shape[0] != t0.shape[0] or t.shape[2:] != t0.shape[2:]:
            raise ValueError(f"{what}: batch / spatial sizes differ: {n0} {tuple(t0.shape)} {name} {tuple(t.shape)}")


def conv3x3x3(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, *, relu: bool = False,
              precision: Optional[str] = None, x2: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
              out_offset: int = 0) -> torch.Tensor:
    """F.conv3d(cat[x, x2], weight, bias, padding=1) (+ ReLU) on the matrix cores, float32 out.  With `out` (a
    contiguous float32 (B, C, H, W, D) tensor) the result goes to its channels [out_offset, out_offset + cout) and
    `out` is returned.  Packs the weights on every call: keep an UpdateBlock where the same weights serve many calls.
    Channel counts outside the kernel's (cin, cout <= 128) run F.conv3d in float32."""
    srcs = (("x", x),) + ((("x2", x2),) if x2 is not None else ()) + ((("out", out),) if out is not None else ())
    _same_volume("conv3x3x3", *srcs)
    cin = x.shape[1] + (0 if x2 is None else x2.shape[1])
    if weight.ndim != 5 or tuple(weight.shape[1:]) != (cin, 3, 3, 3) or tuple(bias.shape) != (weight.shape[0],):
        raise ValueError(f"conv3x3x3: weight {tuple(weight.shape)} bias {tuple(bias.shape)} do not match {cin} input "
                         "channels of a 3 x 3 x 3 convolution")
    cout = int(weight.shape[0])
    if out is not None and not 0 <= out_offset <= out.shape[1] - cout:
        raise ValueError(f"conv3x3x3: channels [{out_offset}, {out_offset + cout}) are not inside out's {out.shape[1]}")
    if out is None and out_offset != 0:
        raise ValueError("conv3x3x3: out_offset needs out")
    ops._need_cuda(*(t for _, t in srcs), weight, bias)
    if _wants_grad(*(t for _, t in srcs), weight, bias):
        raise NotImplementedError("dvccorr.conv3x3x3 has no backward; call it under torch.no_grad() or use F.conv3d "
                                  "for gradients")
    dtype = ops.dtype_code(resolve_precision(x, precision))
    if out is None:
        out = torch.empty((x.shape[0], cout) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("conv3x3x3: out must be contiguous float32")
    x = ops._f32c(x.detach())
    x2 = None if x2 is None else ops._f32c(x2.detach())
    _conv3_layer(None, None, dtype, x, x2, weight, bias, out, out_offset, relu)
    return out


def conv3x3x3_ad(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, *, relu: bool = False,
                 precision: Optional[str] = None, x2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """conv3x3x3 as a differentiable function: F.conv3d(cat[x, x2], weight, bias, padding=1) (+ ReLU) on the matrix
    cores, float32 out (a new tensor), with gradients for x, x2, weight and bias (dvccorr::conv3_ad).  The backward
    runs k_conv3_grad_prep (ReLU mask from the op's own output, bias gradient), k_conv3_wgrad (weight gradient) and
    k_conv3_mfma on the transposed, flipped weights (input gradient), skipping what no input asks for.  Precision as
    conv3x3x3, in both directions: "fp16" / "bf16" round both operands of every product once and accumulate in fp32,
    "fp32" splits them into bf16 hi + lo pieces.  Under "fp16" the incoming gradient is an operand and is rounded to
    fp16 too, as the reference's AMP backward does: scale the loss (GradScaler) so that it stays in fp16's range.
    The packed weights are cached per weight object until it changes (an optimiser step re-packs).  No double
    backward.  Channel counts outside the kernel's (cin, cout <= 128) run F.conv3d in float32 with autograd on."""
    srcs = (("x", x),) + ((("x2", x2),) if x2 is not None else ())
    _same_volume("conv3x3x3", *srcs)
    cin = x.shape[1] + (0 if x2 is None else x2.shape[1])
    if weight.ndim != 5 or tuple(weight.shape[1:]) != (cin, 3, 3, 3) or tuple(bias.shape) != (weight.shape[0],):
        raise ValueError(f"conv3x3x3: weight {tuple(weight.shape)} bias {tuple(bias.shape)} do not match {cin} input "
                         "channels of a 3 x 3 x 3 convolution")
    ops._need_cuda(*(t for _, t in srcs), weight, bias)
    if not conv_covers(cin, int(weight.shape[0])):
        with torch.autocast("cuda", enabled=False):
            xs = x.float() if x2 is None else torch.cat([x.float(), x2.float()], dim=1)
            y = F.conv3d(xs, weight.float(), bias.float(), padding=1)
            return F.relu(y) if relu else y
    dtype = ops.dtype_code(resolve_precision(x, precision))
    return torch.ops.dvccorr.conv3_ad(x, x2, weight, bias, bool(relu), dtype)


def conv7x7x7_flow_ad(flow: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, *,
                      precision: Optional[str] = None) -> torch.Tensor:
    """encoder.convf1 as a differentiable function: relu(F.conv3d(flow, weight, bias, padding=3)) on the matrix cores,
    float32 out (a new tensor), with gradients for weight and bias (dvccorr::conv7_ad).  The backward runs
    k_conv3_grad_prep (ReLU mask from the op's own output, bias gradient) and k_conv7_wgrad (weight gradient),
    skipping what no input asks for.  Precision as conv3x3x3_ad, in both directions; under "fp16" the incoming
    gradient is an operand and is rounded to fp16 too: scale the loss (GradScaler).  The packed weights are cached per
    weight object until it changes.  No double backward.  The model detaches the flow at every iteration
    (raft_dvc.py:441); a flow that does require grad gets torch.nn.grad.conv3d_input of the masked gradient in
    float32, a slow path.  Shapes other than (64, 3, 7, 7, 7) run F.conv3d in float32 with autograd on."""
    _same_volume("conv7x7x7_flow", ("flow", flow))
    if weight.ndim != 5 or tuple(weight.shape[1:]) != (flow.shape[1], 7, 7, 7) or tuple(bias.shape) != (weight.shape[0],):
        raise ValueError(f"conv7x7x7_flow: weight {tuple(weight.shape)} bias {tuple(bias.shape)} do not match "
                         f"{flow.shape[1]} input channels of a 7 x 7 x 7 convolution")
    ops._need_cuda(flow, weight, bias)
    if tuple(weight.shape) != (_lib.CONV7_COUT, 3, 7, 7, 7) or not conv_covers(3, _lib.CONV7_COUT):
        with torch.autocast("cuda", enabled=False):
            return F.relu(F.conv3d(flow.float(), weight.float(), bias.float(), padding=3))
    dtype = ops.dtype_code(resolve_precision(flow, precision))
    return torch.ops.dvccorr.conv7_ad(flow, weight, bias, dtype)


def _block_names(weights, what):
    """(separable, has an uncertainty head, GRU names, all names) of a BasicUpdateBlock.state_dict()."""
    separable = "gru.convz.weight" not in weights
    gru_names = tuple("gru." + n for n in GRU_WEIGHT_NAMES) if separable else _wb(_CONVGRU_LAYERS)
    has_unc = any(n.startswith("uncertainty_head.") for n in weights)
    names = _wb(_ENCODER_LAYERS) + gru_names + _wb(_HEAD_LAYERS) + (_wb(_UNC_LAYERS) if has_unc else ())
    missing = [n for n in names if n not in weights]
    if missing:
        raise ValueError(f"{what}: missing weights {missing} (BasicUpdateBlock.state_dict() names)")
    return separable, has_unc, gru_names, names


def _conv_ad(x, weight, bias, relu, precision, x2=None):
    """A 3 x 3 x 3 layer of update_block_ad: the kernels where they cover it, else F.conv3d in float32 (autograd on)."""
    if tuple(weight.shape[2:]) == (3, 3, 3):
        return conv3x3x3_ad(x, weight, bias, relu=relu, precision=precision, x2=x2)
    with torch.autocast("cuda", enabled=False):
        xs = x.float() if x2 is None else torch.cat([x.float(), x2.float()], dim=1)
        y = F.conv3d(xs, weight.float(), bias.float(), padding=tuple(k // 2 for k in weight.shape[2:]))
        return F.relu(y) if relu else y


def update_block_ad(net: torch.Tensor, context: torch.Tensor, flow: torch.Tensor, weights: Mapping[str, torch.Tensor],
                    *, cor: Optional[torch.Tensor] = None, corr: Optional[torch.Tensor] = None,
                    precision: Optional[str] = None):
    """BasicUpdateBlock.forward (update.py:316-348) as a differentiable function of net, context, cor / corr and every
    parameter in `weights` (the module's state_dict(keep_vars=True) names; the uncertainty head where present):

        net, delta_flow, log_b = update_block_ad(net, context, flow, weights, cor=cor)

    The composition of conv7x7x7_flow_ad (encoder.convf1), conv3x3x3_ad (convf2, conv with x2 = convf2's output, the
    heads), torch.cat([context, motion, flow]) and sep_conv_gru_ad: every convolution runs on the HIP kernels in both
    directions, and the forward values are bit-identical to UpdateBlock's in the same precision.  `cor` is
    relu(convc1(corr)) from lookup_convc1 (differentiable there); a raw `corr` instead runs relu(F.conv3d(corr,
    convc1)) in float32 with autograd on, the slow path.  The flow gets no gradient on the hot path (the model
    detaches coords1, raft_dvc.py:441); one that requires grad takes conv7x7x7_flow_ad's slow path.  A non-separable
    ConvGRU3D, or channel counts outside the kernels', run the float32 library composition with autograd on.  The
    backward keeps the activations of every layer and the GRU's saved gates (sep_conv_gru_ad: 138 MB at 32^3); wrap
    the call in torch.utils.checkpoint(..., use_reentrant=False) to recompute them instead.  No double backward."""
    if (cor is None) == (corr is None):
        raise ValueError("update_block_ad: pass exactly one of cor (= relu(convc1(corr)), from lookup_convc1) and corr")
    separable, has_unc, gru_names, names = _block_names(weights, "update_block_ad")
    feat = ("cor", cor) if cor is not None else ("corr", corr)
    _same_volume("update_block_ad", ("net", net), ("context", context), ("flow", flow), feat)
    w = lambda layer: (weights[layer + ".weight"], weights[layer + ".bias"])   # noqa: E731
    cw = weights["encoder.conv.weight"]
    cor_ch = int(weights["encoder.convc1.weight"].shape[0])
    if flow.shape[1] != 3 or (cor is not None and cor.shape[1] != cor_ch) \
            or cor_ch + weights["encoder.convf2.weight"].shape[0] != cw.shape[1]:
        raise ValueError(f"update_block_ad: flow {tuple(flow.shape)} must have 3 channels and cor {cor_ch} "
                         f"(encoder.conv reads {cw.shape[1]}); got {feat[0]} {tuple(feat[1].shape)}")
    ops._need_cuda(net, context, flow, feat[1], *(weights[n] for n in names))
    precision = resolve_precision(net, precision)
    if cor is None:
        with torch.autocast("cuda", enabled=False):
            cw1, cb1 = w("encoder.convc1")
            cor = F.relu(F.conv3d(corr.float(), cw1.float(), cb1.float()))
    flo1 = conv7x7x7_flow_ad(flow, *w("encoder.convf1"), precision=precision)
    flo2 = _conv_ad(flo1, *w("encoder.convf2"), True, precision)
    mot = _conv_ad(cor, *w("encoder.conv"), True, precision, x2=flo2)
    inp = torch.cat([context.float(), mot, flow.float()], dim=1)
    if separable:
        net = sep_conv_gru_ad(net, inp, {n[4:]: weights[n] for n in gru_names}, precision=precision)
    else:
        with torch.autocast("cuda", enabled=False):
            h = net.float()
            conv = lambda layer, x: F.conv3d(x, *(t.float() for t in w(layer)), padding=1)   # noqa: E731
            hx = torch.cat([h, inp], dim=1)
            z, r = torch.sigmoid(conv("gru.convz", hx)), torch.sigmoid(conv("gru.convr", hx))
            q = torch.tanh(conv("gru.convq", torch.cat([r * h, inp], dim=1)))
            net = (1 - z) * h + z * q

    def head(prefix):
        return _conv_ad(_conv_ad(net, *w(prefix + ".conv1"), True, precision), *w(prefix + ".conv2"), False, precision)
    return net, head("flow_head"), (head("uncertainty_head") if has_unc else None)


class UpdateBlock:
    """BasicUpdateBlock.forward (update.py:316-348) from the module's state_dict(): the motion encoder, the GRU and the
    flow head (and the uncertainty head where the state dict has one).

        net, delta_flow, log_b = block(net, context, flow, cor=cor)

    `cor` is relu(convc1(corr)), which CorrBlock.lookup_convc1 / CorrBlockFused.lookup_convc1 produce with convc1
    fused into the lookup.  A raw `corr` is accepted instead (exactly one of the two): that one 1 x 1 x 1 layer then
    runs as relu(F.conv3d(corr)) in float32 -- the slow path, it reads the whole L (2r + 1)^3-channel tensor.
    log_b is None without an uncertainty head, else the head's raw output (3 channels for "nll", 4 for "mol").

    Packed weights are cached per layer and precision (_PackCache).  The work buffers (convf1's and convf2's outputs,
    the GRU input cat[context, motion features, flow] and the heads' hidden tensor) are cached per
    (B, H, W, D, device), so a captured graph replays on the same addresses; `context` is copied into the GRU input
    only when its storage or version changes, the three flow channels on every call.  Returned tensors are new.

    Layers outside the kernels' shapes (a convf1 that is not 3 -> 64 at 7 x 7 x 7, more than 128 channels in or out,
    a non-separable ConvGRU3D, a GRU other than hidden 96) run as F.conv3d in float32 with autocast disabled.
    Forward only: inputs or weights that require grad (with grad enabled) raise NotImplementedError."""

    def __init__(self, state_dict: Mapping[str, torch.Tensor], precision: Optional[str] = None):
        self.separable, self.has_uncertainty, gru_names, self.names = _block_names(state_dict, "UpdateBlock")
        self.weights = state_dict
        self.precision = precision
        self.gru = SepConvGRU({n[4:]: state_dict[n] for n in gru_names}, precision) if self.separable else None
        self._packed = _PackCache()
        self._buffers: dict = {}

    # -- caches ---------------------------------------------------------------------------------------------------
    def _wbp(self, layer):
        return self.weights[layer + ".weight"], self.weights[layer + ".bias"]

    def _work(self, B, vol, device, ctx_ch):
        key = (B, tuple(vol), device)
        bufs = self._buffers.get(key)
        widths = {"flo1": int(self.weights["encoder.convf1.weight"].shape[0]),
                  "flo2": int(self.weights["encoder.convf2.weight"].shape[0]),
                  "inp": ctx_ch + int(self.weights["encoder.conv.weight"].shape[0]) + 3,
                  "hid": int(self.weights["flow_head.conv1.weight"].shape[0])}
        if self.has_uncertainty:
            widths["hid"] = max(widths["hid"], int(self.weights["uncertainty_head.conv1.weight"].shape[0]))
        if bufs is None or any(bufs[n].shape[1] != c for n, c in widths.items()):
            bufs = {n: torch.empty((B, c) + tuple(vol), dtype=torch.float32, device=device)
                    for n, c in widths.items()}
            bufs["context"] = None
            self._buffers[key] = bufs
        return bufs

    # -- layers ---------------------------------------------------------------------------------------------------
    def _convf1(self, flow, dst, dtype) -> None:
        w, b = self._wbp("encoder.convf1")
        if tuple(w.shape) == (_lib.CONV7_COUT, 3, 7, 7, 7) and conv_covers(3, _lib.CONV7_COUT):
            packed = self._packed.get(("encoder.convf1", dtype), (w, b), lambda: ops.conv7_flow_pack(w, b, dtype))
            torch.ops.dvccorr.conv7_flow(flow, packed, dst, dtype)
        else:
            dst.copy_(_library_conv(flow, w, b, True))

    def _conv3(self, layer, dtype, src0, src1, dst, offset, relu) -> None:
        w, b = self._wbp(layer)
        _conv3_layer(self._packed, layer, dtype, src0, src1, w, b, dst, offset, relu)

    def _head(self, prefix, net, hid, dtype) -> torch.Tensor:
        w1, w2 = self.weights[prefix + ".conv1.weight"], self.weights[prefix + ".conv2.weight"]
        hid = hid if hid.shape[1] == w1.shape[0] else hid[:, :w1.shape[0]].contiguous()
        self._conv3(prefix + ".conv1", dtype, net, None, hid, 0, True)
        out = torch.empty((net.shape[0], int(w2.shape[0])) + tuple(net.shape[2:]), dtype=torch.float32,
                          device=net.device)
        self._conv3(prefix + ".conv2", dtype, hid, None, out, 0, False)
        return out

    def _conv_gru(self, h, x) -> torch.Tensor:
        """The non-separable ConvGRU3D (update.py:118-136) as F.conv3d calls in float32."""
        z = torch.sigmoid(_library_conv(torch.cat([h, x], dim=1), *self._wbp("gru.convz"), False))
        r = torch.sigmoid(_library_conv(torch.cat([h, x], dim=1), *self._wbp("gru.convr"), False))
        q = torch.tanh(_library_conv(torch.cat([r * h, x], dim=1), *self._wbp("gru.convq"), False))
        return (1 - z) * h + z * q

    def __call__(self, net: torch.Tensor, context: torch.Tensor, flow: torch.Tensor,
                 cor: Optional[torch.Tensor] = None, corr: Optional[torch.Tensor] = None):
        if (cor is None) == (corr is None):
            raise ValueError("UpdateBlock: pass exactly one of cor (= relu(convc1(corr)), from lookup_convc1) and corr")
        feat = ("cor", cor) if cor is not None else ("corr", corr)
        _same_volume("UpdateBlock", ("net", net), ("context", context), ("flow", flow), feat)
        cw = self.weights["encoder.conv.weight"]
        cor_ch = int(self.weights["encoder.convc1.weight"].shape[0])
        if flow.shape[1] != 3 or (cor is not None and cor.shape[1] != cor_ch) \
                or cor_ch + self.weights["encoder.convf2.weight"].shape[0] != cw.shape[1]:
            raise ValueError(f"UpdateBlock: flow {tuple(flow.shape)} must have 3 channels and cor {cor_ch} "
                             f"(encoder.conv reads {cw.shape[1]}); got {feat[0]} {tuple(feat[1].shape)}")
        ops._need_cuda(net, context, flow, feat[1], *(self.weights[n] for n in self.names))
        _refuse_grad(net, context, self.weights, self.names, "UpdateBlock", "BasicUpdateBlock", (flow, feat[1]))
        dtype = ops.dtype_code(resolve_precision(net, self.precision))
        with torch.no_grad():
            if cor is None:
                cor = _library_conv(corr, *self._wbp("encoder.convc1"), True)
            cor, flow_c = ops._f32c(cor.detach()), ops._f32c(flow.detach())
            net = ops._f32c(net.detach())
            B, ctx_ch = net.shape[0], int(context.shape[1])
            bufs = self._work(B, net.shape[2:], net.device, ctx_ch)
            inp, mot = bufs["inp"], int(cw.shape[0])
            ctx_state = _PackCache.state([context])
            if bufs["context"] is None or bufs["context"][0] != ctx_state:
                inp[:, :ctx_ch].copy_(context.detach())
                bufs["context"] = (ctx_state, context)
            self._convf1(flow_c, bufs["flo1"], dtype)
            self._conv3("encoder.convf2", dtype, bufs["flo1"], None, bufs["flo2"], 0, True)
            self._conv3("encoder.conv", dtype, cor, bufs["flo2"], inp, ctx_ch, True)
            inp[:, ctx_ch + mot:].copy_(flow_c)
            net = self.gru(net, inp) if self.separable else self._conv_gru(net, inp)
            delta = self._head("flow_head", net, bufs["hid"], dtype)
            log_b = self._head("uncertainty_head", net, bufs["hid"], dtype) if self.has_uncertainty else None
        return net, delta, log_b
