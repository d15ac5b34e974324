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

Inference only: inputs or weights that require grad (with grad enabled) raise NotImplementedError; use the
reference module for gradients.  Training-mode dropout (Dropout3d after conv2, extractor.py:249) is not modelled:
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

__all__ = ["Encoder", "ContextEncoder", "ENCODER_STRIDES", "encoder_strides"]

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
    def _buf(bufs, role, shape, device):
        t = bufs.get((role, shape))
        if t is None:
            t = bufs[(role, shape)] = torch.empty(shape, dtype=torch.float32, device=device)
        return t

    def _conv(self, bufs, role, layer, src, src_ss, prologue, taps, stride, dtype):
        """One raw convolution into the work buffer `role`; with instance norm, its (scale, shift) table too."""
        cout = int(self.sd[layer + ".weight"].shape[0])
        B, ovol = src.shape[0], ops.enc_out_volume(src.shape[2:], stride)
        y = self._buf(bufs, role, (B, cout) + ovol, src.device)
        part = ss = None
        if self.norm == "instance":
            pkey = (role + ".part", (taps, stride, cout) + ovol)
            part = bufs.get(pkey)
            if part is None:
                part = bufs[pkey] = ops.enc_partials(taps, stride, cout, B, ovol, src.device)
            ss = self._buf(bufs, role + ".ss", (B, cout, 2), src.device)
        if taps == _lib.ENC_STEM_TAPS:
            torch.ops.dvccorr.enc_stem(src, self._pack(layer, dtype), y, part, stride, dtype)
        else:
            torch.ops.dvccorr.enc_conv(src, src_ss, prologue, self._pack(layer, dtype), y, None, part, taps, stride,
                                       dtype)
        if ss is not None:
            torch.ops.dvccorr.enc_stats(part, ss, taps, stride, list(ovol), self.eps)
        return y, ss

    def _features(self, x: torch.Tensor, dtype: int):
        """Everything up to conv2's input: the last block's materialised output."""
        B = x.shape[0]
        bufs = self._work(B, x.shape[2:], x.device)
        act = _lib.ENC_NORM_RELU if self.norm == "instance" else _lib.ENC_RELU
        cur, cur_ss = self._conv(bufs, "stem", "conv1", x, None, 0, _lib.ENC_STEM_TAPS, self.strides[0], dtype)
        raw = True   # cur is a raw convolution output (the stem's): its readers apply norm1 + ReLU
        for i, b in enumerate(self.blocks):
            pin = act if raw else _lib.ENC_IDENTITY
            c1, ss1 = self._conv(bufs, "c1", b.name + ".conv1", cur, cur_ss, pin, 1, 1, dtype)
            c2, ss2 = self._conv(bufs, "c2", b.name + ".conv2", c1, ss1, act, 27, b.stride, dtype)
            c3, ss3 = self._conv(bufs, "c3", b.name + ".conv3", c2, ss2, act, 1, 1, dtype)
            if b.down:
                sc, ss4 = self._conv(bufs, "sc", b.down, cur, cur_ss, pin, 1, b.stride, dtype)
                mode = _lib.ENC_SC_NORM
            else:
                sc, ss4, mode = cur, cur_ss, (_lib.ENC_SC_NORM_RELU if raw else _lib.ENC_SC_PLAIN)
            out = self._buf(bufs, f"out{i & 1}", tuple(c3.shape), x.device)
            torch.ops.dvccorr.enc_residual(c3, ss3, sc, ss4, mode, out)
            cur, cur_ss, raw = out, None, False
        return cur

    def _norm(self, x, name):
        sd = self.sd
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

    def _composition(self, x: torch.Tensor) -> torch.Tensor:
        """The reference's layers as library calls in float32 (shapes or norms outside the kernels')."""
        def conv(layer, t, stride, pad):
            w, b = self._wb(layer)
            return F.conv3d(t, w.detach().float(), b.detach().float(), stride=stride, padding=pad)
        with torch.autocast("cuda", enabled=False):
            x = F.relu(self._norm(conv("conv1", x.detach().float(), self.strides[0], 3), "norm1"))
            for b in self.blocks:
                y = F.relu(self._norm(conv(b.name + ".conv1", x, 1, 0), b.name + ".norm1"))
                y = F.relu(self._norm(conv(b.name + ".conv2", y, b.stride, 1), b.name + ".norm2"))
                y = self._norm(conv(b.name + ".conv3", y, 1, 0), b.name + ".norm3")
                r = x if not b.down else self._norm(conv(b.down, x, b.stride, 0), b.name + ".norm4")
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
