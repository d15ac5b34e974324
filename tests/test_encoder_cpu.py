"""CPU: the host layer of dvccorr.Encoder / dvccorr.ContextEncoder (no GPU needed): argument validation and messages,
encoder_type -> strides, from_module on the restated modules, missing-weight errors, the operators' fake
implementations on meta tensors, and the C ABI's host-only size functions and validation."""
from __future__ import annotations

import ctypes

import pytest
import torch
import torch.nn as nn

import raftdvc_encoder as renc

import dvccorr
from dvccorr import _lib, library, ops  # noqa: F401  (registers the ops)
from dvccorr.encoder import ENCODER_STRIDES, encoder_strides


def _sd(kind="1/8", **kw):
    return renc.Encoder(kind, **kw).state_dict()


def test_encoder_type_to_strides():
    assert encoder_strides("1/8") == (2, 1, 2, 2)
    assert encoder_strides("1/4") == (2, 1, 2, 1)
    assert encoder_strides("1/2") == (2, 1, 1, 1)
    assert encoder_strides("1/1") == (1, 1, 1, 1)
    assert encoder_strides("1/2-late-stride") == (1, 1, 1, 2)
    assert encoder_strides([2, 1, 2, 1]) == (2, 1, 2, 1)
    assert set(ENCODER_STRIDES) == {"1/8", "1/4", "1/2", "1/1", "1/2-late-stride"}
    with pytest.raises(ValueError, match="encoder_type must be one of"):
        encoder_strides("1/16")
    with pytest.raises(ValueError, match="four positive integers"):
        encoder_strides((2, 1, 2))
    with pytest.raises(ValueError, match="four positive integers"):
        encoder_strides((2, 1, 0, 1))


def test_argument_validation():
    sd = _sd()
    with pytest.raises(ValueError, match="norm must be one of"):
        dvccorr.Encoder(sd, "1/8", norm="layer")
    with pytest.raises(ValueError, match="missing weights .*conv2.bias"):
        dvccorr.Encoder({k: v for k, v in sd.items() if k != "conv2.bias"}, "1/8")
    # a 1/8 state dict has the same keys as a 1/2 one; a strided block without downsample weights cannot exist, but a
    # state dict whose layer2.0 lost them is caught
    broken = {k: v for k, v in sd.items() if not k.startswith("layer2.0.downsample")}
    with pytest.raises(ValueError, match="no downsample weights"):
        dvccorr.Encoder(broken, "1/8")
    with pytest.raises(ValueError, match="norm='batch' but the state dict has no"):
        dvccorr.Encoder(sd, "1/8", norm="batch")
    with pytest.raises(ValueError, match="missing weights .*encoder.conv1.weight"):
        dvccorr.ContextEncoder(sd, "1/8")           # names without the "encoder." prefix
    csd = {"encoder." + k: v for k, v in _sd(output_dim=160).items()}
    with pytest.raises(ValueError, match="hidden_dim 96 \\+ context_dim 32"):
        dvccorr.ContextEncoder(csd, "1/8", hidden_dim=96, context_dim=32)
    cenc = dvccorr.ContextEncoder(csd, "1/8", norm="none")
    assert (cenc.hidden_dim, cenc.context_dim, cenc.output_dim) == (96, 64, 160) and cenc.kernel_covers()
    enc = dvccorr.Encoder(sd, "1/8")
    with pytest.raises(ValueError, match=r"must be \(B, 1, H, W, D\)"):
        enc(torch.zeros(1, 2, 8, 8, 8))
    with pytest.raises(ValueError, match="empty list"):
        enc([])
    with pytest.raises(RuntimeError, match="MI355X"):   # CPU tensors: no CPU fallback
        enc(torch.zeros(1, 1, 8, 8, 8))


def test_kernel_coverage():
    assert dvccorr.Encoder(_sd(), "1/8", "instance").kernel_covers()
    assert dvccorr.Encoder(_sd(), "1/2-late-stride", "none").kernel_covers()
    assert dvccorr.Encoder(_sd(output_dim=160), "1/4").kernel_covers()
    assert not dvccorr.Encoder(_sd(output_dim=176), "1/4").kernel_covers()      # wider than DVC_ENC_MAX_COUT
    assert not dvccorr.Encoder(_sd(input_dim=2), "1/8").kernel_covers()
    assert not dvccorr.Encoder(_sd(), (4, 1, 2, 2)).kernel_covers()             # a stride the kernels do not have
    assert ops.enc_covers(27, 8, 8) and ops.enc_covers(1, 96, 160)
    assert not ops.enc_covers(27, 12, 8) and not ops.enc_covers(1, 136, 8) and not ops.enc_covers(1, 8, 161)


class _Up(renc.Encoder):
    def forward(self, x):   # an overridden forward, as ShallowUpEncoder's (extractor.py:549-566)
        return super().forward(x) * 2


class _UpEquivalent(_Up):
    sharded_forward_equivalent = True

    def forward(self, x):
        return renc.Encoder.forward(self, x)


def test_from_module():
    for kind in ("1/8", "1/4", "1/2"):
        enc = dvccorr.Encoder.from_module(renc.Encoder(kind).eval())
        assert enc.strides == (2,) + renc.STRIDES[kind] and enc.norm == "instance" and enc.kernel_covers()
    m = renc.Encoder("1/4").eval()
    m.norm1 = nn.Identity()
    assert dvccorr.Encoder.from_module(m).norm == "none"
    m.norm1 = nn.BatchNorm3d(32)            # training mode
    with pytest.raises(NotImplementedError, match="running statistics"):
        dvccorr.Encoder.from_module(m)
    m.norm1 = nn.InstanceNorm3d(32, affine=True)
    with pytest.raises(NotImplementedError, match="norm1 is InstanceNorm3d"):
        dvccorr.Encoder.from_module(m)
    with pytest.raises(NotImplementedError, match="forward is defined by _Up"):
        dvccorr.Encoder.from_module(_Up("1/2").eval())
    assert dvccorr.Encoder.from_module(_UpEquivalent("1/2").eval()).strides == (2, 1, 1, 1)
    with pytest.raises(TypeError, match="has no 'conv1'"):
        dvccorr.Encoder.from_module(nn.Linear(2, 2))
    drop = renc.Encoder("1/2")
    drop.dropout = nn.Dropout3d(0.5)
    with pytest.raises(NotImplementedError, match="dropout in training mode"):
        dvccorr.Encoder.from_module(drop.train())
    # the object holds the module's own parameters, so a later in-place update re-packs
    live = renc.Encoder("1/2").eval()
    assert dvccorr.Encoder.from_module(live).sd["conv2.weight"] is live.conv2.weight

    class Ctx(nn.Module):
        def __init__(self):
            super().__init__()
            self.encoder, self.hidden_dim, self.context_dim = renc.Encoder("1/8", output_dim=160), 96, 64
            self.encoder.norm1 = nn.Identity()
    cenc = dvccorr.ContextEncoder.from_module(Ctx().eval())
    assert (cenc.norm, cenc.hidden_dim, cenc.context_dim, cenc.strides) == ("none", 96, 64, (2, 1, 2, 2))
    with pytest.raises(TypeError, match="has no 'encoder'"):
        dvccorr.ContextEncoder.from_module(renc.Encoder("1/8"))


def test_operators_have_fake_implementations():
    """Shapes and dtypes on meta tensors: the mutating operators return nothing, enc_conv_new allocates conv2's output."""
    f32 = dict(dtype=torch.float32, device="meta")
    x = torch.empty(2, 1, 13, 18, 10, **f32)
    packed = torch.empty(16, **f32)
    y = torch.empty(2, 32, 7, 9, 5, **f32)
    part = torch.empty(8, dtype=torch.float64, device="meta")
    ss = torch.empty(2, 32, 2, **f32)
    assert torch.ops.dvccorr.enc_stem(x, packed, y, part, 2, 0) is None
    assert torch.ops.dvccorr.enc_stats(part, ss, 343, 2, [7, 9, 5], 1e-5) is None
    c1 = torch.empty(2, 8, 7, 9, 5, **f32)
    assert torch.ops.dvccorr.enc_conv(y, ss, 2, packed, c1, None, None, 1, 1, 0) is None
    assert torch.ops.dvccorr.enc_residual(y, ss, y, None, 0, torch.empty_like(y)) is None
    feat = torch.empty(2, 96, 2, 3, 2, **f32)
    out, rest = torch.ops.dvccorr.enc_conv_new(feat, None, 0, packed, 128, -1, 1, 1, 2)
    assert out.shape == (2, 128, 2, 3, 2) and out.dtype == torch.float32 and rest.shape == (2, 0, 2, 3, 2)
    net, ctx = torch.ops.dvccorr.enc_conv_new(feat, None, 0, packed, 160, 96, 1, 2, 1)
    assert net.shape == (2, 96, 1, 2, 1) and ctx.shape == (2, 64, 1, 2, 1) and ctx.dtype == torch.float32


def test_size_functions_and_validation_without_gpu():
    """The C ABI's host logic: packed sizes, the partials size, and argument checks that run before any HIP call."""
    L = _lib.lib()
    frag = 1024
    # 27 taps: cin / 8 chunks of 7 K-steps (27 -> 28 units); 1 tap: 32-channel chunks; tiles padded to the group size
    # (fp32: three bf16 pieces per fragment, 16-bit precisions one)
    assert L.dvc_enc_conv_packed_bytes(27, 8, 8, _lib.DVC_F32) == 7 * 1 * 3 * frag + 16 * 4
    assert L.dvc_enc_conv_packed_bytes(27, 24, 24, _lib.DVC_BF16) == 3 * 7 * 2 * frag + 32 * 4
    assert L.dvc_enc_conv_packed_bytes(1, 96, 160, _lib.DVC_F16) == 3 * 12 * frag + 192 * 4
    assert L.dvc_enc_conv_packed_bytes(1, 24, 96, _lib.DVC_F32) == 1 * 8 * 3 * frag + 128 * 4
    assert L.dvc_enc_stem_packed_bytes(_lib.DVC_F32) == 11 * 2 * 3 * frag + 32 * 4
    assert L.dvc_enc_stem_packed_bytes(7) == 0
    for bad in ((27, 12, 8), (1, 136, 8), (1, 8, 161), (9, 8, 8), (27, 0, 8)):
        assert L.dvc_enc_conv_packed_bytes(*bad, _lib.DVC_F32) == 0, bad
    # boxes of 4 x 4 x 16 output voxels, 4 x 2 x 16 for the strided 3 x 3 x 3 layers; two doubles per channel
    assert L.dvc_enc_partials_bytes(343, 2, 32, 2, 7, 9, 5) == 2 * (2 * 3 * 1) * 32 * 16
    assert L.dvc_enc_partials_bytes(27, 2, 8, 2, 5, 3, 9) == 2 * (2 * 2 * 1) * 8 * 16
    assert L.dvc_enc_partials_bytes(27, 1, 8, 2, 5, 3, 9) == 2 * (2 * 1 * 1) * 8 * 16
    assert L.dvc_enc_partials_bytes(27, 3, 8, 2, 5, 3, 9) == 0 and L.dvc_enc_partials_bytes(1, 1, 8, 0, 5, 3, 9) == 0
    p = ctypes.c_void_p(4096)
    assert L.dvc_enc_stem(None, p, p, None, 1, 8, 8, 8, 2, 0, None) == _lib.DVC_ERR_INVALID
    assert L.dvc_enc_stem(p, p, ctypes.c_void_p(1 << 30), None, 1, 8, 8, 8, 3, 0, None) == _lib.DVC_ERR_INVALID
    assert L.dvc_enc_conv(p, None, 0, p, None, None, -1, None, 27, 1, 8, 8, 1, 8, 8, 8, 0, None) == _lib.DVC_ERR_INVALID
    far = ctypes.c_void_p(1 << 30)
    assert L.dvc_enc_conv(p, None, 3, p, far, None, -1, None, 27, 1, 8, 8, 1, 8, 8, 8, 0, None) == _lib.DVC_ERR_INVALID
    assert L.dvc_enc_conv(p, None, 0, p, far, None, -1, None, 27, 1, 12, 8, 1, 8, 8, 8, 0, None) == _lib.DVC_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError, match="cin a multiple of 8"):
        _lib.check(_lib.DVC_ERR_UNSUPPORTED)
    assert L.dvc_enc_conv(p, None, 0, p, far, None, 8, None, 1, 1, 8, 8, 1, 8, 8, 8, 0, None) == _lib.DVC_ERR_INVALID
    assert L.dvc_enc_conv(p, None, 0, p, p, None, -1, None, 1, 1, 8, 8, 1, 8, 8, 8, 0, None) == _lib.DVC_ERR_INVALID
    with pytest.raises(ValueError, match="must not overlap"):
        _lib.check(_lib.DVC_ERR_INVALID)
    assert L.dvc_enc_stats(None, p, 1, 1, 8, 1, 8, 8, 8, 1e-5, None) == _lib.DVC_ERR_INVALID
    assert L.dvc_enc_residual(p, None, p, None, 0, p, 8, 1, 8, 8, 8, None) == _lib.DVC_ERR_INVALID
    assert L.dvc_enc_residual(p, None, p, None, 5, far, 8, 1, 8, 8, 8, None) == _lib.DVC_ERR_INVALID
    assert L.dvc_enc_residual(p, None, p, None, 0, far, 40000, 2, 8, 8, 8, None) == _lib.DVC_ERR_UNSUPPORTED
