"""GPU: dvccorr.Encoder / dvccorr.ContextEncoder (csrc/encoder.hip) against the reference's fixtures, the float64
restatement of the encoders (tests/raftdvc_encoder.py) and float64 F.conv3d per layer.

Whole-encoder tolerances.  Metric: max |err| / max |ref| against the float64 restatement on the CPU.
  fp16 / bf16   the yardstick is the same nn.Module on the GPU under torch.autocast of that dtype, against the same
                float64 result; the HIP error may be at most 2 x the yardstick's (the rounding points are the same or
                fewer, activations stay in float32; the factor covers accumulation order).
  fp32          twice the largest value measured over the cases of tests 1-3, but never above 1e-4 = ten times the
                per-layer bound the project holds elsewhere.  Measured on the MI355X: fixture 1/8
                5.29e-6, 1/4 4.71e-6, 1/2 2.64e-6; ceil shapes 1/8 2.76e-6, 1/2 4.16e-6; norm 'none' (context encoder)
                2.7e-7.  ENC_FP32_TOL = 1.1e-5 is twice the largest, rounded up.  (With two bf16 pieces per fp32
                operand, as the update block's kernels use, the same cases measured 6.3e-5 to 1.11e-4: the 2^-17
                operand error compounds through the twenty instance-normalised layers.  The encoder kernels
                therefore split fp32 operands into three pieces.)
Per-layer bounds are the project's standing ones (FWD_TOL of tests/test_gpu_conv3_grad.py).
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import prng
import raftdvc_encoder as renc
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PRECISIONS = ("fp32", "fp16", "bf16")
FWD_TOL = {"fp32": 1e-5, "fp16": 1e-2, "bf16": 1e-2}   # per layer (tests/test_gpu_conv3_grad.py)
AUTOCAST = {"fp16": torch.float16, "bf16": torch.bfloat16}
ENC_FP32_TOL = 1.1e-5   # 2 x the largest measured fp32 whole-encoder error (5.29e-6, fixture 1/8), rounded up


def _rel(got, ref):
    ref = ref.double().cpu()
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


def _identity_norms(enc):
    """The restated encoder with norm_fn = 'none' (extractor.py:121-122): every norm an nn.Identity."""
    enc.norm1 = nn.Identity()
    for layer in (enc.layer1, enc.layer2, enc.layer3):
        for blk in layer:
            blk.norm1, blk.norm2, blk.norm3 = nn.Identity(), nn.Identity(), nn.Identity()
            if blk.downsample is not None:
                blk.norm4 = nn.Identity()
                blk.downsample[1] = blk.norm4
    return enc


@functools.lru_cache(maxsize=None)
def _model(kind, norm, output_dim, seed0):
    enc = renc.Encoder(kind, output_dim=output_dim).eval()
    if norm == "none":
        _identity_norms(enc)
    renc.set_params(enc, seed0)
    return enc


@functools.lru_cache(maxsize=None)
def _case(kind, norm, output_dim, seed0, in_seed, shape):
    """(module, input, float64 CPU output of the restatement), computed once and shared."""
    enc = _model(kind, norm, output_dim, seed0)
    x = torch.from_numpy(prng.uniform(in_seed, shape))
    with torch.no_grad():
        ref = enc.double()(x.double())
        enc.float()
    return enc, x, ref


def _sd(enc, prefix=""):
    return {prefix + k: v.detach().to(DEV) for k, v in enc.state_dict().items()}


@functools.lru_cache(maxsize=None)
def _yardstick(kind, norm, output_dim, seed0, in_seed, shape, precision):
    """Error of the same nn.Module on the GPU under autocast, against the float64 result."""
    enc, x, ref = _case(kind, norm, output_dim, seed0, in_seed, shape)
    mod = _model(kind, norm, output_dim, seed0)
    import copy
    gpu = copy.deepcopy(mod).to(DEV)
    with torch.no_grad(), torch.autocast("cuda", dtype=AUTOCAST[precision]):
        y = gpu(x.to(DEV))
    return _rel(y.float(), ref)


def _check_whole(got, key, precision, label):
    ref = _case(*key)[2]
    err = _rel(got, ref)
    if precision == "fp32":
        print(f"encoder {label} fp32: rel err {err:.3e} (bound {ENC_FP32_TOL:.1e})")
        assert err <= ENC_FP32_TOL, (label, err)
    else:
        yard = _yardstick(*key, precision)
        print(f"encoder {label} {precision}: rel err {err:.3e}, autocast yardstick {yard:.3e}")
        assert err <= 2 * yard, (label, precision, err, yard)


# ---------------------------------------------------------------------------------------------------------------
# test 1: the reference's fixtures
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tag", ["1_8", "1_4", "1_2"])
def test_reference_fixture(tag, precision):
    import dvccorr
    g = load_golden(f"encoder_{tag}.npz")
    kind = {"1_8": "1/8", "1_4": "1/4", "1_2": "1/2"}[tag]
    key = (kind, "instance", 128, int(g["seed0"][0]), int(g["in_seed"][0]), tuple(int(v) for v in g["in_shape"]))
    mod, x, ref64 = _case(*key)
    gold = torch.from_numpy(g["out"])
    assert _rel(ref64, gold) < 1e-5          # the float64 restatement is the fixture's network
    enc = dvccorr.Encoder(_sd(mod), encoder_type=kind, norm="instance", precision=precision)
    assert enc.kernel_covers()
    out = enc(x.to(DEV))
    assert out.shape == gold.shape and out.dtype == torch.float32
    _check_whole(out, key, precision, f"fixture {tag}")
    if precision == "fp32":                  # the float32 reference output itself
        assert _rel(out, gold) <= ENC_FP32_TOL + 1e-5   # + the fixture's own float32 error against float64


# ---------------------------------------------------------------------------------------------------------------
# test 2: odd extents at every stride-2 layer, partial tiles on every axis, B = 2
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", ["1/8", "1/2"])
def test_ceil_shapes_and_pair_call(kind, precision):
    import dvccorr
    key = (kind, "instance", 128, 9100, 9101, (2, 1, 13, 18, 10))
    mod, x, ref = _case(*key)
    enc = dvccorr.Encoder(_sd(mod), encoder_type=kind, norm="instance", precision=precision)
    xg = x.to(DEV)
    out = enc(xg)
    assert tuple(out.shape) == tuple(ref.shape)
    _check_whole(out, key, precision, f"ceil {kind}")
    # instance norm is per sample: the pair call equals two single calls bit for bit
    f0, f1 = enc([xg[:1], xg[1:]])
    s0, s1 = enc(xg[:1]), enc(xg[1:])
    assert torch.equal(f0, s0) and torch.equal(f1, s1)
    assert torch.equal(torch.cat([f0, f1]), out)


# ---------------------------------------------------------------------------------------------------------------
# test 3: norm = 'none' and the context encoder
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_context_encoder(precision):
    import dvccorr
    g = load_golden("context_encoder_1_8.npz")
    hidden, ctx = int(g["hidden_dim"][0]), int(g["context_dim"][0])
    key = ("1/8", "none", hidden + ctx, int(g["seed0"][0]), int(g["in_seed"][0]), tuple(int(v) for v in g["in_shape"]))
    mod, x, ref = _case(*key)
    ref_net, ref_ctx = torch.tanh(ref[:, :hidden]), F.relu(ref[:, hidden:])
    # the float64 restatement with identity norms is the reference's ContextEncoder
    assert _rel(ref_net, torch.from_numpy(g["net"])) < 1e-5 and _rel(ref_ctx, torch.from_numpy(g["context"])) < 1e-5
    cenc = dvccorr.ContextEncoder(_sd(mod, "encoder."), encoder_type="1/8", norm="none", hidden_dim=hidden,
                                  context_dim=ctx, precision=precision)
    assert cenc.kernel_covers()
    net, context = cenc(x.to(DEV))
    assert net.shape == ref_net.shape and context.shape == ref_ctx.shape
    assert float(net.abs().max()) < 1.0 and float(context.min()) >= 0.0
    # the pre-activation error bound carries over: tanh and ReLU are 1-Lipschitz; the metric stays relative to the
    # float64 pre-activation maximum
    scale = float(ref.abs().max())
    err = max(float((net.double().cpu() - ref_net).abs().max()), float((context.double().cpu() - ref_ctx).abs().max())) / scale
    if precision == "fp32":
        print(f"encoder context fp32: rel err {err:.3e} (bound {ENC_FP32_TOL:.1e})")
        assert err <= ENC_FP32_TOL, err
    else:
        yard = _yardstick(*key, precision)
        print(f"encoder context {precision}: rel err {err:.3e}, autocast yardstick {yard:.3e}")
        assert err <= 2 * yard, (err, yard)
    # the plain encoder with norm = 'none' returns the pre-activation
    enc = dvccorr.Encoder(_sd(mod), encoder_type="1/8", norm="none", precision=precision)
    _check_whole(enc(x.to(DEV)), key, precision, "norm none")


# ---------------------------------------------------------------------------------------------------------------
# test 4: one layer per kernel against float64 F.conv3d
# ---------------------------------------------------------------------------------------------------------------
VOL = (9, 6, 17)


def _uniform(seed, shape, lo=-1.0, hi=1.0):
    return torch.from_numpy(prng.uniform(seed, tuple(shape), lo, hi))


def _shell_and_interior(err):
    """Max of |err| (B, C, H, W, D) over the one-voxel border shell and over the interior."""
    m = torch.zeros(err.shape[2:], dtype=torch.bool)
    m[0], m[-1], m[:, 0], m[:, -1], m[:, :, 0], m[:, :, -1] = True, True, True, True, True, True
    shell = float(err[:, :, m].max())
    inner = float(err[:, :, ~m].max()) if (~m).any() else 0.0
    return shell, inner


def _assert_layer(got, ref, precision, label):
    lim = FWD_TOL[precision] * float(ref.abs().max())
    shell, inner = _shell_and_interior((got.double().cpu() - ref).abs())
    print(f"{label} {precision}: shell {shell:.3e} interior {inner:.3e} (bound {lim:.3e})")
    assert shell <= lim, (label, "border shell", shell, lim)
    assert inner <= lim, (label, "interior", inner, lim)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("stride", [1, 2])
def test_stem_layer(stride, precision):
    from dvccorr import ops
    dt = ops.dtype_code(precision)
    x = _uniform(7000 + stride, (2, 1) + VOL)
    w, b = _uniform(7010, (32, 1, 7, 7, 7), -343 ** -0.5, 343 ** -0.5), _uniform(7011, (32,), -0.5, 0.5)
    ref = F.conv3d(x.double(), w.double(), b.double(), stride=stride, padding=3)
    y = torch.empty(ref.shape, dtype=torch.float32, device=DEV)
    part = ops.enc_partials(343, stride, 32, 2, ref.shape[2:], DEV)
    ops.enc_stem(x.to(DEV), ops.enc_stem_pack(w.to(DEV), b.to(DEV), dt), y, part, stride, dt)
    _assert_layer(y, ref, precision, f"stem stride {stride}")
    # its statistics: scale = 1 / sqrt(var + eps), shift = -mean scale
    ss = torch.empty((2, 32, 2), dtype=torch.float32, device=DEV)
    ops.enc_stats(part, ss, 343, stride, ref.shape[2:], 1e-5)
    y64 = y.double().cpu().flatten(2)
    inv = (y64.var(dim=2, unbiased=False) + 1e-5).rsqrt()
    want = torch.stack([inv, -y64.mean(dim=2) * inv], dim=2)
    assert float((ss.double().cpu() - want).abs().max()) <= 1e-6 * float(want.abs().max())


CONV_CASES = [  # (taps, stride, cin, cout, split)
    (27, 1, 8, 8, -1), (27, 2, 8, 8, -1), (27, 1, 24, 24, -1), (27, 2, 24, 24, -1),
    (1, 1, 32, 8, -1), (1, 1, 24, 96, -1), (1, 2, 64, 96, -1), (1, 1, 96, 160, 96),
]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("taps,stride,cin,cout,split", CONV_CASES)
def test_conv_layer(taps, stride, cin, cout, split, precision):
    """Every prologue.  Prologue 2 uses shift = +2 on inputs in [-1, 1] with scales in [0.5, 1.5], so relu(shift) = 2
    everywhere: a padding tap that wrongly received the prologue would be off by order one at the border shell."""
    from dvccorr import ops
    dt = ops.dtype_code(precision)
    k = 3 if taps == 27 else 1
    seed = 7100 + 10 * cin + stride + taps
    x = _uniform(seed, (2, cin) + VOL)
    bound = (cin * taps) ** -0.5
    w, b = _uniform(seed + 1, (cout, cin, k, k, k), -bound, bound), _uniform(seed + 2, (cout,), -0.5, 0.5)
    ss = torch.stack([_uniform(seed + 3, (2, cin), 0.5, 1.5), torch.full((2, cin), 2.0)], dim=2).contiguous()
    packed = ops.enc_conv_pack(w.to(DEV), b.to(DEV), dt)
    for prologue in (0, 1, 2):
        xin = x.double()
        if prologue == 2:
            xin = xin * ss[:, :, 0].double()[:, :, None, None, None] + ss[:, :, 1].double()[:, :, None, None, None]
        if prologue:
            xin = F.relu(xin)
        ref = F.conv3d(xin, w.double(), b.double(), stride=stride, padding=k // 2)
        ovol = tuple(ref.shape[2:])
        part = ops.enc_partials(taps, stride, cout, 2, ovol, DEV)
        label = f"taps {taps} stride {stride} {cin}->{cout} prologue {prologue}"
        if split < 0:
            y = torch.empty(ref.shape, dtype=torch.float32, device=DEV)
            ops.enc_conv(x.to(DEV), ss.to(DEV) if prologue == 2 else None, prologue, packed, y, None, part, taps,
                         stride, dt)
            _assert_layer(y, ref, precision, label)
        else:
            y = torch.empty((2, split) + ovol, dtype=torch.float32, device=DEV)
            y2 = torch.empty((2, cout - split) + ovol, dtype=torch.float32, device=DEV)
            ops.enc_conv(x.to(DEV), ss.to(DEV) if prologue == 2 else None, prologue, packed, y, y2, part, taps,
                         stride, dt)
            lim = FWD_TOL[precision] * float(ref.abs().max())   # tanh and ReLU are 1-Lipschitz
            assert float((y.double().cpu() - torch.tanh(ref[:, :split])).abs().max()) <= lim, label
            assert float((y2.double().cpu() - F.relu(ref[:, split:])).abs().max()) <= lim, label
            assert float(y.abs().max()) < 1.0 and float(y2.min()) >= 0.0
        # the partials are the sums of the raw output the kernel stored
        sums = part.view(2, -1, cout, 2).sum(dim=1).cpu()
        assert float((sums[..., 0] - ref.flatten(2).sum(dim=2)).abs().max()) <= \
            FWD_TOL[precision] * float(ref.abs().max()) * ref[0, 0].numel()


# ---------------------------------------------------------------------------------------------------------------
# test 5: statistics
# ---------------------------------------------------------------------------------------------------------------
def test_statistics_survive_a_large_mean():
    """A unit-variance output around +100 over 4,096 voxels: a float32 E[x^2] - E[x]^2 loses about 6e-4 of the variance
    there (x^2 ~ 1e4 carries 24 bits), far above the fp32 per-layer bound; double sums do not.  The layer is the
    identity on bf16-representable inputs, so the convolution itself is exact and the statistics are what is tested;
    the consumer is k_enc_residual with a zero shortcut."""
    from dvccorr import ops
    dt = ops.dtype_code("fp32")
    vol, C = (16, 16, 16), 8
    x = torch.from_numpy(prng.normal(7300, (1, C) + vol)).bfloat16().float()
    w = torch.eye(C).reshape(C, C, 1, 1, 1).contiguous()
    b = torch.full((C,), 100.0)
    y = torch.empty((1, C) + vol, dtype=torch.float32, device=DEV)
    part = ops.enc_partials(1, 1, C, 1, vol, DEV)
    ops.enc_conv(x.to(DEV), None, 0, ops.enc_conv_pack(w.to(DEV), b.to(DEV), dt), y, None, part, 1, 1, dt)
    ss = torch.empty((1, C, 2), dtype=torch.float32, device=DEV)
    ops.enc_stats(part, ss, 1, 1, vol, 1e-5)
    out = torch.empty_like(y)
    ops.enc_residual(y, ss, torch.zeros_like(y), None, 0, out)
    y64 = (x.double() + 100.0).flatten(2)
    mean, var = y64.mean(dim=2, keepdim=True), y64.var(dim=2, unbiased=False, keepdim=True)
    ref = F.relu((y64 - mean) / (var + 1e-5).sqrt()).reshape(out.shape)
    err, lim = float((out.double().cpu() - ref).abs().max()), FWD_TOL["fp32"] * float(ref.abs().max())
    print(f"statistics at mean 100: err {err:.3e} (bound {lim:.3e})")
    assert err <= lim, (err, lim)
    # what a float32 sum of squares would have given: outside the bound, so the test separates the two schemes
    y32 = (x + 100.0).flatten(2)
    var32 = (y32 * y32).sum(dim=2, keepdim=True, dtype=torch.float32) / y32.shape[2] - y32.mean(dim=2, keepdim=True) ** 2
    bad = F.relu((y64 - mean) / (var32.double() + 1e-5).sqrt()).reshape(out.shape)
    assert float((bad - ref).abs().max()) > lim


def test_two_runs_are_bit_identical():
    import dvccorr
    key = ("1/8", "instance", 128, 9100, 9101, (2, 1, 13, 18, 10))
    mod, x, _ = _case(*key)
    xg = x.to(DEV)
    a = dvccorr.Encoder(_sd(mod), "1/8", "instance", precision="fp32")(xg)
    b = dvccorr.Encoder(_sd(mod), "1/8", "instance", precision="fp32")(xg)
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------
# test 6: fallbacks, refusals, caches, graph capture
# ---------------------------------------------------------------------------------------------------------------
def _batch_norms(enc, seed):
    g = torch.Generator().manual_seed(seed)

    def bn(c):
        m = nn.BatchNorm3d(c)
        with torch.no_grad():
            m.running_mean.copy_(torch.randn(c, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(c, generator=g) + 0.5)
            m.weight.copy_(torch.rand(c, generator=g) + 0.5)
            m.bias.copy_(torch.randn(c, generator=g) * 0.1)
        return m
    enc.norm1 = bn(32)
    for layer in (enc.layer1, enc.layer2, enc.layer3):
        for blk in layer:
            mid, planes = blk.conv1.out_channels, blk.conv3.out_channels
            blk.norm1, blk.norm2, blk.norm3 = bn(mid), bn(mid), bn(planes)
            if blk.downsample is not None:
                blk.norm4 = bn(planes)
                blk.downsample[1] = blk.norm4
    return enc.eval()


def test_library_path_for_uncovered_encoders():
    import dvccorr
    x = _uniform(7400, (1, 1, 16, 12, 8)).to(DEV)
    mod = renc.Encoder("1/4")
    renc.set_params(mod, 7401)
    mod = _batch_norms(mod, 7402).to(DEV)
    enc = dvccorr.Encoder(mod.state_dict(), "1/4", norm="batch")
    assert not enc.kernel_covers()
    with torch.no_grad():
        want = mod(x)
        assert _rel(enc(x), want) <= 1e-5
        assert _rel(dvccorr.Encoder.from_module(mod)(x), want) <= 1e-5
    mod2 = renc.Encoder("1/2", input_dim=2).eval()
    renc.set_params(mod2, 7403)
    mod2 = mod2.to(DEV)
    x2 = _uniform(7404, (1, 2, 16, 12, 8)).to(DEV)
    enc2 = dvccorr.Encoder(mod2.state_dict(), "1/2", norm="instance")
    assert not enc2.kernel_covers()
    with torch.no_grad():
        assert _rel(enc2(x2), mod2(x2)) <= 1e-5


def test_grad_refused_and_weights_repack():
    import dvccorr
    key = ("1/2", "instance", 128, 9100, 9101, (1, 1, 16, 12, 8))
    mod, x, _ = _case(*key)
    sd = _sd(mod)
    enc = dvccorr.Encoder(sd, "1/2", "instance", precision="fp32")
    with pytest.raises(NotImplementedError, match="BasicEncoder"):
        enc(x.to(DEV).requires_grad_(True))
    live = dvccorr.Encoder.from_module(_model(*key[:4]).to(DEV))   # parameters require grad
    try:
        with pytest.raises(NotImplementedError, match="BasicEncoder"):
            live(x.to(DEV))
        with torch.no_grad():
            assert torch.equal(live(x.to(DEV)), enc(x.to(DEV)))
    finally:
        _model(*key[:4]).cpu()
    a = enc(x.to(DEV))
    sd["conv2.bias"].add_(1.0)            # in place: the version counter re-packs
    b = enc(x.to(DEV))
    assert float((b - a - 1.0).abs().max()) < 1e-5


def test_graph_capture_replays():
    import dvccorr
    key = ("1/8", "instance", 128, 9100, 9101, (2, 1, 13, 18, 10))
    mod, x, _ = _case(*key)
    enc = dvccorr.Encoder(_sd(mod), "1/8", "instance", precision="fp16")
    xg = x.to(DEV)
    eager = enc(xg).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        enc(xg)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = enc(xg)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
