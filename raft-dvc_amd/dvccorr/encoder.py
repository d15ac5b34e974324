"""The feature and context encoders on the MI355X: BasicEncoder / MediumEncoder / ShallowEncoder / LateStrideEncoder /
FullResEncoder.forward and ContextEncoder.forward (src/core/extractor.py:142-301, raft_dvc.py:360-367, 423-427).

    enc  = dvccorr.Encoder(model.fnet.state_dict(), encoder_type="1/8", norm="instance")   # once per weight set
    fmap0, fmap1 = enc([vol0, vol1])          # list / tuple -> batch-concatenated, split again; a tensor -> a tensor
    cenc = dvccorr.ContextEncoder(model.cnet.state_dict(), encoder_type="1/8", norm="none",
                                  hidden_dim=96, context_dim=64)
    net, context = cenc(vol0)                 # tanh on the first hidden_dim channels, relu on the rest
    enc  = dvccorr.Encoder.from_module(model.fnet)   # reads strides and norm classes from the module tree

The encoder classes of the reference have identical state dicts and differ only in strides, and InstanceNorm3d /
Identity leave no keys, so `encoder_type` ('1/8', '1/4', '1/2', '1/1', '1/2-late-stride', or the strides
(conv1, layer1, layer2, layer3)) and `norm` are explicit.

The kernels (csrc/encoder.hip) store every convolution's raw output once, in float32; its InstanceNorm3d (eps 1e-5,
biased variance, no affine) and ReLU are applied by the kernel that reads it, so no pass exists only to normalise:
k_enc_stem (conv1), k_enc_conv (the bottleneck's three convolutions, the strided shortcut, conv2), k_enc_stats
(per-(b, c) scale and shift from double-precision partial sums, fixed order: two runs are bit-identical) and
k_enc_residual (relu(norm3(c3) + shortcut), the only place a block output is materialised).  Precision follows
resolve_precision: "fp16" / "bf16" (also inside a CUDA autocast region) round the MFMA operands once and accumulate
in fp32; "fp32" splits them into three bf16 pieces (the float32 value exactly, six products per step: two pieces, as
the update block uses, compound to 1e-4 through the twenty normalised layers).  Activations between kernels,
statistics and outputs are float32 in every precision.

They cover input_dim 1, the bottleneck layout of extractor.py:79-139 with the reference's widths (a 32-channel
7 x 7 x 7 conv1, convolution inputs a multiple of 8 up to 128 channels), norms 'instance' and 'none', strides 1 and
2 and output widths up to 160.  Anything else (batch and group norm, another input width) runs the library
composition (F.conv3d and the functional norms, eval-mode statistics) in float32 with autocast disabled.

Measured on an MI355X against the same nn.Module (tools/bench_encoder.py): 4.4x (fnet pair) and 2.8x
(cnet) faster at 256^3 in fp32, 4.1x / 2.1x in fp16, 2-3x at 128^3.  At 64^3 the fp32 path is NOT measurably faster
(1.30 ms against 1.40 in one run, 1.24 against 1.22 in another): the call is 53 launches and is bound by the host's
launch path, not by the kernels; capture the call in a graph there.  The fp32 whole-encoder error against float64 is
2.6e-6 to 5.3e-6 with instance norm (2.7e-7 without).

Encoder and ContextEncoder are inference only: inputs or weights that require grad (with grad enabled) raise
NotImplementedError.  Training goes through encoder_ad(x | [x0, x1], module.state_dict(keep_vars=True), ...) and
context_encoder_ad(x, ...): the same kernels in the same order into new tensors (forward values bit-identical), every
raw output, table and block output kept in float32, and the backward of csrc/encoder_grad.hip: the
instance norm's gradient and the bias sums from double partials in a fixed order, dW on k_enc_wgrad (MFMA, split-K
over the voxels), the input gradient on k_enc_conv with transposed, flipped weights (a strided layer through its
zero-inserted source mode).  The input volume is data: it gets no gradient.  Training-mode dropout (Dropout3d after conv2, extractor.py:249) is not modelled:
the objects compute the eval-mode forward.
"""
from __future__ import annotations

from typing import Mapping, Optional, Sequence, Tuple, Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, library, ops  # noqa: F401  (library registers the operators)
from .corr_block import _wants_grad, resolve_precision
from .update import _PackCache

__all__ = ["Encoder", "ContextEncoder", "ENCODER_STRIDES", "encoder_strides", "encoder_ad", "context_encoder_ad"]

#: encoder_type -> strides of (conv1, layer1, layer2, layer3): BasicEncoder, MediumEncoder, ShallowEncoder,
#: FullResEncoder and LateStrideEncoder (extractor.py:168-176, 336-344, 447-455, 607-615, 541-545)
ENCODER_STRIDES = {"1/8": (2, 1, 2, 2), "1/4": (2, 1, 2, 1), "1/2": (2, 1, 1, 1), "1/1": (1, 1, 1, 1),
                   "1/2-late-stride": (1, 1, 1, 2)}
NORMS = ("instance", "none", "batch", "group")
_EPS = 1e-5
#: classes whose forward is conv1 -> norm1 -> relu -> layers -> conv2 (the sequence the kernels run)
KNOWN_FORWARDS = ("BasicEncoder", "MediumEncoder", "ShallowEncoder", "FullResEncoder")


def encoder_strides(encoder_type: Union[str, Sequence[int]]) -> Tuple[int, int, int, int]:
    """The (conv1, layer1, layer2, layer3) strides of an encoder_type name, or the validated tuple itself."""
    if isinstance(encoder_type, str):
        if encoder_type not in ENCODER_STRIDES:
            raise ValueError(f"encoder_type must be one of {sorted(ENCODER_STRIDES)} or a (conv1, layer1, layer2, "
                             f"layer3) strides tuple, got {encoder_type!r}")
        return ENCODER_STRIDES[encoder_type]
    s = tuple(int(v) for v in encoder_type)
    if len(s) != 4 or any(v < 1 for v in s):
        raise ValueError(f"encoder strides must be four positive integers (conv1, layer1, layer2, layer3), got "
                         f"{tuple(encoder_type)!r}")
    return s


class _Block:
    """One BottleneckBlock3D of the state dict: layer names, stride and channel counts."""

    def __init__(self, sd, name, stride, what):
        self.name, self.stride = name, stride
        self.down = f"{name}.downsample.0" if f"{name}.downsample.0.weight" in sd else None
        cin, mid = int(sd[f"{name}.conv1.weight"].shape[1]), int(sd[f"{name}.conv1.weight"].shape[0])
        planes = int(sd[f"{name}.conv3.weight"].shape[0])
        shapes = {"conv1": (mid, cin, 1, 1, 1), "conv2": (mid, mid, 3, 3, 3), "conv3": (planes, mid, 1, 1, 1)}
        if self.down:
            shapes["downsample.0"] = (planes, cin, 1, 1, 1)
        for l, shp in shapes.items():
            if tuple(sd[f"{name}.{l}.weight"].shape) != shp:
                raise ValueError(f"{what}: {name}.{l}.weight is {tuple(sd[f'{name}.{l}.weight'].shape)}, a "
                                 f"BottleneckBlock3D's would be {shp}")
        if self.down is None and (stride != 1 or cin != planes):
            raise ValueError(f"{what}: {name} has stride {stride} and {cin} -> {planes} channels but no downsample "
                             "weights (wrong encoder_type for this state dict?)")
        self.cin, self.mid, self.planes = cin, mid, planes


class Encoder:
    """A RAFT-DVC feature encoder's eval-mode forward from its state_dict() (module docstring).

    Packed weights are cached per layer and precision (_PackCache: an in-place update or a replaced tensor re-packs).
    Work buffers are cached per (B, H, W, D, device), so a captured graph replays on the same addresses; returned
    tensors are new.  `prefix` selects the names inside a larger state dict (ContextEncoder uses "encoder.")."""

    reference = "BasicEncoder"

    def __init__(self, state_dict: Mapping[str, torch.Tensor], encoder_type: Union[str, Sequence[int]] = "1/8",
                 norm: str = "instance", precision: Optional[str] = None, prefix: str = "", eps: float = _EPS):
        what = type(self).__name__
        self.strides = encoder_strides(encoder_type)
        if norm not in NORMS:
            raise ValueError(f"{what}: norm must be one of {NORMS}, got {norm!r}")
        self.norm, self.precision, self.eps = norm, precision, float(eps)
        sd = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
        blocks = [f"layer{i}.{j}" for i in (1, 2, 3) for j in (0, 1)]
        convs = ["conv1"] + [f"{b}.{c}" for b in blocks for c in ("conv1", "conv2", "conv3")] + ["conv2"]
        missing = [f"{prefix}{n}.{k}" for n in convs for k in ("weight", "bias") if f"{n}.{k}" not in sd]
        if missing:
            raise ValueError(f"{what}: missing weights {missing} ({self.reference}.state_dict() names)")
        self.sd = sd
        self.blocks = [_Block(sd, b, self.strides[int(b[5])] if b.endswith(".0") else 1, what) for b in blocks]
        self.input_dim = int(sd["conv1.weight"].shape[1])
        self.output_dim = int(sd["conv2.weight"].shape[0])
        self.names = tuple(f"{n}.{k}" for n in convs + [b.down for b in self.blocks if b.down]
                           for k in ("weight", "bias"))
        if norm in ("batch", "group"):
            norms = ["norm1"] + [f"{b.name}.norm{i}" for b in self.blocks for i in (1, 2, 3, 4) if i < 4 or b.down]
            need = ("weight", "bias") + (("running_mean", "running_var") if norm == "batch" else ())
            missing = [f"{prefix}{n}.{k}" for n in norms for k in need if f"{n}.{k}" not in sd]
            if missing:
                raise ValueError(f"{what}: norm={norm!r} but the state dict has no {missing[:4]} ...")
        self._packed = _PackCache()
        self._buffers: dict = {}

    # -- construction from a module ---------------------------------------------------------------------------------
    @staticmethod
    def _module_structure(enc: nn.Module, what: str):
        for name in ("conv1", "norm1", "conv2", "layer1", "layer2", "layer3"):
            if not hasattr(enc, name):
                raise TypeError(f"{what}.from_module: the module has no {name!r} (expected a RAFT-DVC feature encoder)")
        owner = next((k for k in type(enc).__mro__ if "forward" in vars(k)), None)
        if not (owner is not None and (owner.__name__ in KNOWN_FORWARDS
                                       or vars(owner).get("sharded_forward_equivalent", False))):
            raise NotImplementedError(
                f"{what}.from_module: {type(enc).__name__}.forward is defined by {getattr(owner, '__name__', None)}, "
                f"not by one of {KNOWN_FORWARDS}; a forward that adds steps (e.g. ShallowUpEncoder's x2 upsample) "
                "would be skipped")
        if getattr(enc, "training", False) and getattr(enc, "dropout", None) is not None:
            raise NotImplementedError(f"{what}.from_module: dropout in training mode is not modelled; call .eval()")
        n1 = enc.norm1
        if isinstance(n1, nn.InstanceNorm3d) and not n1.affine and not n1.track_running_stats:
            norm = "instance"
        elif isinstance(n1, nn.Identity):
            norm = "none"
        elif isinstance(n1, nn.BatchNorm3d):
            if n1.training or not n1.track_running_stats:
                raise NotImplementedError(f"{what}.from_module: BatchNorm3d runs with its running statistics here; "
                                          "call .eval() on a module that tracks them")
            norm = "batch"
        elif isinstance(n1, nn.GroupNorm):
            norm = "group"
        else:
            raise NotImplementedError(f"{what}.from_module: norm1 is {type(n1).__name__}; InstanceNorm3d without "
                                      "affine parameters, Identity, BatchNorm3d and GroupNorm are supported")
        strides = (enc.conv1.stride[0],) + tuple(getattr(enc, f"layer{i}")[0].conv2.stride[0] for i in (1, 2, 3))
        return strides, norm, float(getattr(n1, "eps", _EPS))

    @classmethod
    def from_module(cls, module: nn.Module, precision: Optional[str] = None) -> "Encoder":
        """An Encoder on the module's own parameter tensors (a later optimiser step or load_state_dict re-packs):
        strides and norm kind are read from the module tree.  A class whose forward is not the reference's conv1 ->
        norm1 -> relu -> layers -> conv2 sequence is refused unless it sets `sharded_forward_equivalent = True`."""
        strides, norm, eps = cls._module_structure(module, cls.__name__)
        return cls(module.state_dict(keep_vars=True), strides, norm, precision, eps=eps)

    # -- dispatch ---------------------------------------------------------------------------------------------------
    def kernel_covers(self) -> bool:
        """The kernels run this encoder (else the float32 library composition does)."""
        sd = self.sd
        if self.norm not in ("instance", "none") or any(s not in (1, 2) for s in self.strides):
            return False
        if tuple(sd["conv1.weight"].shape) != (_lib.ENC_STEM_COUT, 1, 7, 7, 7):
            return False
        cin = _lib.ENC_STEM_COUT
        for b in self.blocks:
            if b.cin != cin or not (ops.enc_covers(1, b.cin, b.mid) and ops.enc_covers(27, b.mid, b.mid)
                                    and ops.enc_covers(1, b.mid, b.planes) and ops.enc_covers(1, b.cin, b.planes)):
                return False
            cin = b.planes
        w2 = sd["conv2.weight"]
        return tuple(w2.shape[1:]) == (cin, 1, 1, 1) and ops.enc_covers(1, cin, int(w2.shape[0]))

    def _wb(self, layer):
        return self.sd[layer + ".weight"], self.sd[layer + ".bias"]

    def _pack(self, layer, dtype):
        w, b = self._wb(layer)
        pack = ops.enc_stem_pack if layer == "conv1" else ops.enc_conv_pack
        return self._packed.get((layer, dtype), (w, b), lambda: pack(w, b, dtype))

    def _work(self, B, vol, device):
        key = (B, tuple(vol), device)
        return self._buffers.setdefault(key, {})

    @staticmethod
    def _buf(bufs, role, shape, device, keep=None):
        if keep is not None:   # the training forward: every tensor the backward reads is a new one
            return torch.empty(shape, dtype=torch.float32, device=device)
        t = bufs.get((role, shape))
        if t is None:
            t = bufs[(role, shape)] = torch.empty(shape, dtype=torch.float32, device=device)
        return t

    def _conv(self, bufs, role, layer, src, src_ss, prologue, taps, stride, dtype, keep=None):
        """One raw convolution into the work buffer `role`; with instance norm, its (scale, shift) table too.  With
        `keep` (the training forward) both are new tensors, recorded as keep[layer] and keep[layer + ".ss"]."""
        cout = int(self.sd[layer + ".weight"].shape[0])
        B, ovol = src.shape[0], ops.enc_out_volume(src.shape[2:], stride)
        y = self._buf(bufs, role, (B, cout) + ovol, src.device, keep)
        part = ss = None
        if self.norm == "instance":
            pkey = (role + ".part", (taps, stride, cout) + ovol)
            part = bufs.get(pkey)
            if part is None:
                part = bufs[pkey] = ops.enc_partials(taps, stride, cout, B, ovol, src.device)
            ss = self._buf(bufs, role + ".ss", (B, cout, 2), src.device, keep)
        if taps == _lib.ENC_STEM_TAPS:
            torch.ops.dvccorr.enc_stem(src, self._pack(layer, dtype), y, part, stride, dtype)
        else:
            torch.ops.dvccorr.enc_conv(src, src_ss, prologue, self._pack(layer, dtype), y, None, part, taps, stride,
                                       dtype)
        if ss is not None:
            torch.ops.dvccorr.enc_stats(part, ss, taps, stride, list(ovol), self.eps)
        if keep is not None:
            keep[layer] = y
            if ss is not None:
                keep[layer + ".ss"] = ss
        return y, ss

    def _features(self, x: torch.Tensor, dtype: int, keep=None):
        """Everything up to conv2's input: the last block's materialised output.  With `keep`, the same launches in
        the same order into new tensors: every raw output, table and block output (keep[block + ".out"]) stays."""
        B = x.shape[0]
        bufs = self._work(B, x.shape[2:], x.device)
        act = _lib.ENC_NORM_RELU if self.norm == "instance" else _lib.ENC_RELU
        cur, cur_ss = self._conv(bufs, "stem", "conv1", x, None, 0, _lib.ENC_STEM_TAPS, self.strides[0], dtype, keep)
        raw = True   # cur is a raw convolution output (the stem's): its readers apply norm1 + ReLU
        for i, b in enumerate(self.blocks):
            pin = act if raw else _lib.ENC_IDENTITY
            c1, ss1 = self._conv(bufs, "c1", b.name + ".conv1", cur, cur_ss, pin, 1, 1, dtype, keep)
            c2, ss2 = self._conv(bufs, "c2", b.name + ".conv2", c1, ss1, act, 27, b.stride, dtype, keep)
            c3, ss3 = self._conv(bufs, "c3", b.name + ".conv3", c2, ss2, act, 1, 1, dtype, keep)
            if b.down:
                sc, ss4 = self._conv(bufs, "sc", b.down, cur, cur_ss, pin, 1, b.stride, dtype, keep)
                mode = _lib.ENC_SC_NORM
            else:
                sc, ss4, mode = cur, cur_ss, (_lib.ENC_SC_NORM_RELU if raw else _lib.ENC_SC_PLAIN)
            out = self._buf(bufs, f"out{i & 1}", tuple(c3.shape), x.device, keep)
            torch.ops.dvccorr.enc_residual(c3, ss3, sc, ss4, mode, out)
            if keep is not None:
                keep[b.name + ".out"] = out
            cur, cur_ss, raw = out, None, False
        return cur

    def _norm(self, x, name, grad=False):
        sd = self.sd
        if grad and self.norm in ("batch", "group"):   # the library path of encoder_ad: the affine parameters train too
            if self.norm == "batch":
                return F.batch_norm(x, sd[name + ".running_mean"].detach().float(), sd[name + ".running_var"].detach().float(),
                                    sd[name + ".weight"].float(), sd[name + ".bias"].float(), False, 0.0, self.eps)
            return F.group_norm(x, max(1, x.shape[1] // 8), sd[name + ".weight"].float(), sd[name + ".bias"].float(),
                                self.eps)
        if self.norm == "instance":
            return F.instance_norm(x, eps=self.eps)
        if self.norm == "batch":
            return F.batch_norm(x, sd[name + ".running_mean"].detach().float(), sd[name + ".running_var"].detach().float(),
                                sd[name + ".weight"].detach().float(), sd[name + ".bias"].detach().float(), False, 0.0,
                                self.eps)
        if self.norm == "group":
            return F.group_norm(x, max(1, x.shape[1] // 8), sd[name + ".weight"].detach().float(),
                                sd[name + ".bias"].detach().float(), self.eps)
        return x

    def _composition(self, x: torch.Tensor, grad: bool = False) -> torch.Tensor:
        """The reference's layers as library calls in float32 (shapes or norms outside the kernels').  `grad`: the
        weights are not detached (encoder_ad's slow path, under autograd)."""
        def conv(layer, t, stride, pad):
            w, b = self._wb(layer)
            if not grad:
                w, b = w.detach(), b.detach()
            return F.conv3d(t, w.float(), b.float(), stride=stride, padding=pad)
        with torch.autocast("cuda", enabled=False):
            x = F.relu(self._norm(conv("conv1", x.detach().float(), self.strides[0], 3), "norm1", grad))
            for b in self.blocks:
                y = F.relu(self._norm(conv(b.name + ".conv1", x, 1, 0), b.name + ".norm1", grad))
                y = F.relu(self._norm(conv(b.name + ".conv2", y, b.stride, 1), b.name + ".norm2", grad))
                y = self._norm(conv(b.name + ".conv3", y, 1, 0), b.name + ".norm3", grad)
                r = x if not b.down else self._norm(conv(b.down, x, b.stride, 0), b.name + ".norm4", grad)
                x = F.relu(y + r)
            return conv("conv2", x, 1, 0)

    def _check(self, x: torch.Tensor) -> None:
        what = type(self).__name__
        if not isinstance(x, torch.Tensor) or x.ndim != 5 or x.shape[1] != self.input_dim:
            raise ValueError(f"{what}: the input must be (B, {self.input_dim}, H, W, D), got "
                             f"{tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
        ws = [self.sd[n] for n in self.names]
        ops._need_cuda(x, *ws)
        if _wants_grad(x, *ws):
            raise NotImplementedError(f"dvccorr.{what} has no backward; call it under torch.no_grad() or use the "
                                      f"reference's {self.reference} for gradients")

    def _run(self, x: torch.Tensor, split: int):
        self._check(x)
        with torch.no_grad():
            if not self.kernel_covers():
                y = self._composition(x)
                return (y, None) if split < 0 else (torch.tanh(y[:, :split]), F.relu(y[:, split:]))
            dtype = ops.dtype_code(resolve_precision(x, self.precision))
            feat = self._features(ops._f32c(x.detach()), dtype)
            y, y2 = torch.ops.dvccorr.enc_conv_new(feat, None, _lib.ENC_IDENTITY, self._pack("conv2", dtype),
                                                   self.output_dim, split, 1, 1, dtype)
            return y, (None if split < 0 else y2)

    def __call__(self, x):
        """BasicEncoder.forward: a tensor, or a list / tuple of tensors that is concatenated along the batch and split
        again (extractor.py:232-256)."""
        if isinstance(x, (tuple, list)):
            if not x:
                raise ValueError(f"{type(self).__name__}: an empty list of volumes")
            sizes = [int(t.shape[0]) for t in x]
            return torch.split(self._run(torch.cat(list(x), dim=0), -1)[0], sizes, dim=0)
        return self._run(x, -1)[0]


class ContextEncoder(Encoder):
    """ContextEncoder.forward (extractor.py:259-301) from its state_dict() (names prefixed "encoder."): the encoder,
    then tanh on the first hidden_dim output channels and ReLU on the other context_dim, fused into conv2's
    epilogue and written to two new tensors.  Everything else as Encoder."""

    reference = "ContextEncoder"

    def __init__(self, state_dict: Mapping[str, torch.Tensor], encoder_type: Union[str, Sequence[int]] = "1/8",
                 norm: str = "none", hidden_dim: int = 96, context_dim: int = 64, precision: Optional[str] = None,
                 prefix: str = "encoder.", eps: float = _EPS):
        super().__init__(state_dict, encoder_type, norm, precision, prefix, eps)
        if hidden_dim < 1 or context_dim < 1 or hidden_dim + context_dim != self.output_dim:
            raise ValueError(f"ContextEncoder: hidden_dim {hidden_dim} + context_dim {context_dim} must be conv2's "
                             f"{self.output_dim} output channels")
        self.hidden_dim, self.context_dim = int(hidden_dim), int(context_dim)

    @classmethod
    def from_module(cls, module: nn.Module, precision: Optional[str] = None) -> "ContextEncoder":
        if not hasattr(module, "encoder"):
            raise TypeError("ContextEncoder.from_module: the module has no 'encoder' (expected a RAFT-DVC ContextEncoder)")
        strides, norm, eps = cls._module_structure(module.encoder, cls.__name__)
        return cls(module.state_dict(keep_vars=True), strides, norm, int(module.hidden_dim), int(module.context_dim),
                   precision, eps=eps)

    def __call__(self, x: torch.Tensor):
        return self._run(x, self.hidden_dim)


# ---------------------------------------------------------------------------------------------------------------
# training: encoder_ad / context_encoder_ad (backward: csrc/encoder_grad.hip)
# ---------------------------------------------------------------------------------------------------------------
_N_CONVS = 20   # conv1, six blocks x three, conv2


def _ad_names(weights, strides):
    """State-dict names of a flat weight list in Encoder.names order (the twenty convolutions, then the shortcut
    convolutions of the blocks that have one)."""
    names = ["conv1"] + [f"layer{i}.{j}.{c}" for i in (1, 2, 3) for j in (0, 1) for c in ("conv1", "conv2", "conv3")] + \
        ["conv2"]
    if len(weights) < 2 * _N_CONVS or len(weights) % 2:
        raise ValueError(f"encoder_ad: {len(weights)} weight tensors; an encoder has at least {2 * _N_CONVS}")
    cin = int(weights[0].shape[0])
    for k, blk in enumerate(f"layer{i}.{j}" for i in (1, 2, 3) for j in (0, 1)):
        planes = int(weights[2 * (3 + 3 * k)].shape[0])
        stride = strides[1 + k // 2] if k % 2 == 0 else 1
        if stride != 1 or cin != planes:
            names.append(blk + ".downsample.0")
        cin = planes
    if len(names) * 2 != len(weights):
        raise ValueError(f"encoder_ad: {len(weights)} weight tensors for {len(names)} convolutions")
    return [f"{n}.{k}" for n in names for k in ("weight", "bias")]


def _ad_encoder(weights, strides, instance, eps) -> "Encoder":
    """The Encoder (structure, one _PackCache for the forward and the dgrad packs) of a flat weight list.  It lives on
    the weight set itself, as an attribute of its first tensor (conv1.weight), so calls between optimiser steps do not
    re-pack, an in-place step re-packs (_PackCache), and the packs and work buffers go when the weights go (the
    reference cycle tensor -> Encoder -> tensor is the garbage collector's).  Nothing is kept process-wide."""
    key = (tuple(strides), bool(instance), float(eps))
    slot = getattr(weights[0], "_dvc_ad_encoders", None)
    if slot is None:
        slot = weights[0]._dvc_ad_encoders = {}
    enc = slot.get(key)
    if enc is None or len(enc._ad_weights) != len(weights) or any(a is not b for a, b in zip(enc._ad_weights, weights)):
        enc = Encoder(dict(zip(_ad_names(weights, strides), weights)), tuple(strides), "instance" if instance else "none",
                      eps=eps)
        enc._ad_weights = list(weights)
        slot[key] = enc
    return enc


def _ad_kept_names(enc: "Encoder"):
    """The tensors the training forward keeps, in the order dvccorr::encoder_ad returns them."""
    inst = enc.norm == "instance"
    names = []
    def layer(n):
        names.append(n)
        if inst:
            names.append(n + ".ss")
    layer("conv1")
    for b in enc.blocks:
        for c in ("conv1", "conv2", "conv3"):
            layer(f"{b.name}.{c}")
        if b.down:
            layer(b.down)
        names.append(b.name + ".out")
    return names


def _ad_forward(x, weights, strides, instance, split, eps, dtype):
    """dvccorr::encoder_ad: [y, y2, *kept]."""
    enc = _ad_encoder(weights, strides, instance, eps)
    keep: dict = {}
    with torch.no_grad():
        feat = enc._features(ops._f32c(x.detach()), dtype, keep)
        y, y2 = torch.ops.dvccorr.enc_conv_new(feat, None, _lib.ENC_IDENTITY, enc._pack("conv2", dtype), enc.output_dim,
                                               split, 1, 1, dtype)
    return [y, y2] + [keep[n] for n in _ad_kept_names(enc)]


def _ad_fake(x, weights, strides, instance, split):
    names = _ad_names(weights, strides)
    sh = {n: tuple(w.shape) for n, w in zip(names, weights)}
    B, vol = x.shape[0], tuple(x.shape[2:])
    new = lambda *s: x.new_empty(s, dtype=torch.float32)
    kept = []
    def layer(n, v):
        kept.append(new(B, sh[n + ".weight"][0], *v))
        if instance:
            kept.append(new(B, sh[n + ".weight"][0], 2))
    vol = ops.enc_out_volume(vol, strides[0])
    layer("conv1", vol)
    for k, blk in enumerate(f"layer{i}.{j}" for i in (1, 2, 3) for j in (0, 1)):
        stride = strides[1 + k // 2] if k % 2 == 0 else 1
        layer(blk + ".conv1", vol)
        vol = ops.enc_out_volume(vol, stride)
        layer(blk + ".conv2", vol)
        layer(blk + ".conv3", vol)
        if blk + ".downsample.0.weight" in sh:
            layer(blk + ".downsample.0", vol)
        kept.append(new(B, sh[blk + ".conv3.weight"][0], *vol))
    cout = sh["conv2.weight"][0]
    return [new(B, cout if split < 0 else split, *vol), new(B, 0 if split < 0 else cout - split, *vol)] + kept


def _ad_backward(x, weights, strides, instance, split, eps, dtype, outs, g_y, g_y2, need):
    """The backward of dvccorr::encoder_ad: the layers in reverse.  Per layer: the norm's gradient g_x (and db) in one
    elementwise pass pair (enc_norm_grad), dW on k_enc_wgrad from the stored raw input and the forward's prologue, the
    input gradient on k_enc_conv with the dgrad pack; the residual's two paths meet in enc_grad_add.  Whatever
    `need` does not ask for, and everything upstream of the first layer that asks, is skipped."""
    enc = _ad_encoder(weights, strides, instance, eps)
    names = list(enc.names)
    need = dict(zip(names, need))
    kept = dict(zip(_ad_kept_names(enc), outs[2:]))
    grads = {}
    order = {"conv1": 0, "conv2": 1 + 4 * len(enc.blocks)}
    for i, b in enumerate(enc.blocks):
        order.update({f"{b.name}.conv1": 1 + 4 * i, f"{b.name}.conv2": 2 + 4 * i, f"{b.name}.conv3": 3 + 4 * i})
        if b.down:
            order[b.down] = 1 + 4 * i
    first = min((order[n.rsplit(".", 1)[0]] for n in names if need[n]), default=None)
    if first is None:
        return [None] * len(names)
    act = _lib.ENC_NORM_RELU if instance else _lib.ENC_RELU
    O = torch.ops.dvccorr

    def upstream(layer):   # a layer before this one asks: this layer's input gradient is needed
        return first < order[layer]

    def norm_grad(layer, g, mask):
        """g with respect to the layer's normalised output (before the consumer's ReLU mask) -> g_x; records db."""
        nb = need[layer + ".bias"]
        ss = kept.get(layer + ".ss")
        if ss is None and not mask:
            if nb:
                grads[layer + ".bias"] = O.enc_norm_grad(g, None, None, False, False, True)[1]
            return g
        gx, db = O.enc_norm_grad(g, kept[layer], ss, mask, True, nb)
        if nb:
            grads[layer + ".bias"] = db
        return gx

    def layer_back(layer, gx, src, src_ss, prologue, taps, stride):
        w = enc.sd[layer + ".weight"]
        if need[layer + ".weight"]:
            grads[layer + ".weight"] = O.enc_wgrad(src, src_ss if prologue == _lib.ENC_NORM_RELU else None, prologue, gx,
                                                   taps, stride, dtype)
        if not upstream(layer):
            return None
        packed = enc._packed.get(("dgrad", layer, dtype), (w,), lambda: ops.enc_conv_pack_dgrad(w, dtype))
        return O.enc_dgrad(gx, packed, taps, stride, int(w.shape[1]), list(src.shape[2:]), dtype)

    # the inputs of every block, as the forward saw them
    ins, cur, cur_ss, raw = [], kept["conv1"], kept.get("conv1.ss"), True
    for b in enc.blocks:
        ins.append((cur, cur_ss, raw))
        cur, cur_ss, raw = kept[b.name + ".out"], None, False

    if split >= 0:
        g = O.enc_split_grad(g_y, g_y2, outs[0], outs[1])
    else:
        g = g_y
    g = norm_grad("conv2", g, False)
    g = layer_back("conv2", g, cur, None, _lib.ENC_IDENTITY, 1, 1)
    for b, (cur, cur_ss, raw) in zip(reversed(enc.blocks), reversed(ins)):
        if g is None:
            break
        n1, n2, n3 = (f"{b.name}.conv{k}" for k in (1, 2, 3))
        pin = act if raw else _lib.ENC_IDENTITY
        g_pre = O.enc_grad_add(g, None, kept[b.name + ".out"])
        g3 = norm_grad(n3, g_pre, False)
        # conv3, conv2, conv1: the chain ends at the first layer that asks (its input gradient is None)
        ga = layer_back(n3, g3, kept[n2], kept.get(n2 + ".ss"), act, 1, 1)
        if ga is not None:
            ga = layer_back(n2, norm_grad(n2, ga, True), kept[n1], kept.get(n1 + ".ss"), act, 27, b.stride)
        g_in = None
        if ga is not None:
            g_in = layer_back(n1, norm_grad(n1, ga, True), cur, cur_ss, pin, 1, 1)
        g_sc = g_pre
        if b.down:
            g_sc = None
            if need[b.down + ".weight"] or need[b.down + ".bias"] or upstream(b.down):
                g_sc = layer_back(b.down, norm_grad(b.down, g_pre, False), cur, cur_ss, pin, 1, b.stride)
        g = None if g_in is None or g_sc is None else O.enc_grad_add(g_in, g_sc, None)
    if g is not None:   # the stem: relu(norm1(conv1(x)))
        gs = norm_grad("conv1", g, True)
        if need["conv1.weight"]:
            grads["conv1.weight"] = O.enc_wgrad(ops._f32c(x.detach()), None, _lib.ENC_IDENTITY, gs, _lib.ENC_STEM_TAPS,
                                                strides[0], dtype)
    out = []
    for n, w in zip(names, weights):
        gw = grads.get(n)
        out.append(None if gw is None else gw.reshape(w.shape).to(w.dtype))
    return out


def _ad_call(what, x, weights, encoder_type, norm, precision, prefix, eps, split, keep):
    if isinstance(x, torch.Tensor) and x.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError(f"dvccorr.{what}: the input volume requires grad, but it is data here: the encoders' "
                                  "backward has no input-volume gradient (detach the volume)")
    probe = Encoder(weights, encoder_type, norm, precision, prefix, eps)   # validates names, shapes, norm
    if not isinstance(x, torch.Tensor) or x.ndim != 5 or x.shape[1] != probe.input_dim:
        raise ValueError(f"{what}: the input must be (B, {probe.input_dim}, H, W, D), got "
                         f"{tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
    ws = [probe.sd[n] for n in probe.names]
    ops._need_cuda(x, *ws)
    covered = probe.kernel_covers() and all(
        ops.enc_grad_covers(27 if w.shape[2] == 3 else 1, int(w.shape[1]), int(w.shape[0]))
        for n, w in zip(probe.names, ws) if n.endswith(".weight") and n != "conv1.weight")
    if not covered:   # the slow path: the library composition in float32 under autograd
        y = probe._composition(x, grad=True)
        return (y, None) if split < 0 else (torch.tanh(y[:, :split]), F.relu(y[:, split:]))
    dtype = ops.dtype_code(resolve_precision(x, precision))
    outs = torch.ops.dvccorr.encoder_ad(x, ws, list(probe.strides), norm == "instance", split, float(eps), dtype)
    if keep is not None:
        enc = _ad_encoder(ws, probe.strides, norm == "instance", float(eps))
        keep.update(zip(_ad_kept_names(enc), (t.detach() for t in outs[2:])))
    return outs[0], (None if split < 0 else outs[1])


def encoder_ad(x, weights: Mapping[str, torch.Tensor], encoder_type: Union[str, Sequence[int]] = "1/8",
               norm: str = "instance", precision: Optional[str] = None, prefix: str = "", eps: float = _EPS,
               keep: Optional[dict] = None):
    """A feature encoder's forward that trains: every convolution weight and bias of `weights`
    (module.state_dict(keep_vars=True)) that requires grad gets a gradient, on HIP in both directions
    (dvccorr::encoder_ad; backward csrc/encoder_grad.hip).  A tensor in, a tensor out; a list / tuple of volumes is
    concatenated along the batch and split again.  The forward values are bit-identical to dvccorr.Encoder's in the
    same precision: the same kernels run in the same order, but into new tensors.

    Kept for the backward, all float32: every raw convolution output, every (scale, shift) table and every block
    output, i.e. roughly the sum of all layer outputs: 4 B (OH OW OD at conv1's stride) x about 200 channel-volumes at
    '1/8' -- about 30 MB for a 64^3 pair, 240 MB at 128^3.  16-bit storage of these stays open.

    The input volume is data: a volume that requires grad raises NotImplementedError.  No double backward.  Eval-mode
    semantics (no dropout).  Precision follows resolve_precision in both directions: "fp16" / "bf16" round both
    operands of every product once and accumulate in fp32, "fp32" splits them into three bf16 pieces.  Under "fp16"
    the incoming gradients are operands and are rounded too: scale the loss as under AMP.  Encoders kernel_covers()
    rejects (batch or group norm, other widths) run the library composition in float32 under autograd (slow).
    `keep` is a test hook: a dict that receives the kept tensors by layer name ("layer1.0.conv2",
    "layer1.0.conv2.ss", "layer1.0.out", ...), without copies."""
    if isinstance(x, (tuple, list)):
        if not x:
            raise ValueError("encoder_ad: an empty list of volumes")
        if any(t.requires_grad for t in x) and torch.is_grad_enabled():
            raise NotImplementedError("dvccorr.encoder_ad: an input volume requires grad, but it is data here: the "
                                      "encoders' backward has no input-volume gradient (detach the volume)")
        sizes = [int(t.shape[0]) for t in x]
        y = _ad_call("encoder_ad", torch.cat(list(x), dim=0), weights, encoder_type, norm, precision, prefix, eps, -1, keep)[0]
        return torch.split(y, sizes, dim=0)
    return _ad_call("encoder_ad", x, weights, encoder_type, norm, precision, prefix, eps, -1, keep)[0]


def context_encoder_ad(x, weights: Mapping[str, torch.Tensor], encoder_type: Union[str, Sequence[int]] = "1/8",
                       norm: str = "none", hidden_dim: int = 96, context_dim: int = 64, precision: Optional[str] = None,
                       prefix: str = "encoder.", eps: float = _EPS, keep: Optional[dict] = None):
    """ContextEncoder.forward that trains: (net, context) = (tanh, relu) halves of the encoder's output, every
    convolution weight and bias that requires grad gets a gradient.  Everything else as encoder_ad."""
    w2 = weights.get(prefix + "conv2.weight")
    if w2 is None or hidden_dim < 1 or context_dim < 1 or hidden_dim + context_dim != int(w2.shape[0]):
        raise ValueError(f"context_encoder_ad: hidden_dim {hidden_dim} + context_dim {context_dim} must be conv2's output "
                         "channels")
    return _ad_call("context_encoder_ad", x, weights, encoder_type, norm, precision, prefix, eps, int(hidden_dim), keep)
