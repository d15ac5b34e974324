"""GPU: dvccorr.encoder_ad / context_encoder_ad (csrc/encoder_grad.hip) against the float64 restatement of the encoders
(tests/encoder_grad.py) run on the HIP run's own ReLU masks, and per layer against float64 F.conv3d autograd.

Metric: max |err| / max |ref| per parameter tensor (update_cases.err); for a bias under an instance norm, whose
gradient is exactly zero, |err| / max_c sum |g_x| of the float64 run.
Bounds of the whole-encoder test (set against references, never against the code under test):
  the yardstick is the same network as library calls on the GPU (float32, or torch.autocast of the 16-bit dtype),
  recording its own masks and compared with float64 on its own record;
  fp16 / bf16   per tensor, HIP error <= 2 x the yardstick's;
  fp32          per tensor, HIP error <= min(1e-4, max(1e-5, 2 x yardstick));
  mask agreement between the float64 run's own pre > 0 and the HIP masks is printed for every precision and asserted
  (>= 0.999 per ReLU) in fp32 only.
Per-layer bounds are the project's standing ones (tests/test_gpu_conv3_grad.py): fp32 1e-5, 16-bit 1e-2.
Measured values: DESIGN.md 4.17.
"""
from __future__ import annotations

import functools

import pytest
import torch
import torch.nn.functional as F

import encoder_grad as eg
import prng

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PRECISIONS = ("fp32", "fp16", "bf16")
LAYER_TOL = {"fp32": 1e-5, "fp16": 1e-2, "bf16": 1e-2}
AUTOCAST = {"fp16": torch.float16, "bf16": torch.bfloat16}
DT = {"fp32": 0, "bf16": 1, "fp16": 2}
AGREE_MIN = 0.999

CASES = {
    "A": dict(ctx=False, kind="1/8", norm="instance", vols=[(1, 13, 18, 10), (1, 13, 18, 10)], out=128, seed=4100),
    "B": dict(ctx=True, kind="1/8", norm="none", vols=[(2, 13, 18, 10)], out=160, seed=4300),
    "C": dict(ctx=False, kind="1/1", norm="instance", vols=[(1, 9, 6, 17)], out=128, seed=4500),
}
HIDDEN = 96


def _rand(seed, shape):
    return torch.from_numpy(prng.uniform(seed, tuple(shape), -1.0, 1.0))


def _err(a, ref):
    ref = ref.double().cpu()
    return float((a.double().cpu() - ref).abs().max() / ref.abs().max())


def _inputs(case):
    c = CASES[case]
    return [_rand(c["seed"] + 900 + i, (v[0], 1) + v[1:]) for i, v in enumerate(c["vols"])]


def _loss(case, outs, dtype, device):
    """A fixed functional of the outputs with prng tensors G: G-weighted means (a sum over a 1/1 encoder's 10^5 output
    values times the fp16 loss scale of 1024 leaves the fp16 range in the library yardstick and in the kernels alike)."""
    c = CASES[case]
    G = lambda k, t: _rand(c["seed"] + 950 + k, t.shape).to(device=device, dtype=dtype) / t.numel()
    if case == "A":
        return (outs[0].to(dtype) * outs[1].to(dtype) * G(0, outs[0])).sum()
    if case == "B":
        return (outs[0].to(dtype) * G(0, outs[0])).sum() + (outs[1].to(dtype) * G(1, outs[1])).sum()
    return (outs[0].to(dtype) * G(0, outs[0])).sum()


def _restated(case, sd, xs, tape):
    c = CASES[case]
    strides = eg.STRIDES[c["kind"]]
    x = torch.cat(xs, dim=0)
    if c["ctx"]:
        return list(eg.context_encoder(x, sd, strides, HIDDEN, c["norm"], tape))
    y = eg.encoder(x, sd, strides, c["norm"], tape)
    return list(torch.split(y, [t.shape[0] for t in xs], dim=0))


def _f64_on(case, masks, scale):
    """Float64 gradients on the CPU with the given masks; (grads, tape)."""
    c = CASES[case]
    prefix = "encoder." if c["ctx"] else ""
    sd = eg.leaves(_weights(case), torch.float64, "cpu")
    tape = eg.Tape(masks)
    outs = _restated(case, sd, [x.double() for x in _inputs(case)], tape)
    (_loss(case, outs, torch.float64, "cpu") * scale).backward()
    return {n: w.grad for n, w in sd.items()}, tape, prefix


@functools.lru_cache(maxsize=None)
def _weights(case):
    c = CASES[case]
    return eg.make_weights(eg.STRIDES[c["kind"]], c["out"], c["seed"], "encoder." if c["ctx"] else "")


def _hip(case, precision, sd, keep=None):
    import dvccorr
    c = CASES[case]
    xs = [x.float().to(DEV) for x in _inputs(case)]
    if c["ctx"]:
        return list(dvccorr.context_encoder_ad(xs[0], sd, c["kind"], c["norm"], HIDDEN, c["out"] - HIDDEN, precision,
                                               keep=keep))
    return list(dvccorr.encoder_ad(xs, sd, c["kind"], c["norm"], precision, keep=keep))


@functools.lru_cache(maxsize=None)
def _run(case, precision):
    """(HIP errors, yardstick errors, HIP mask agreement) per parameter / ReLU."""
    c = CASES[case]
    scale = 1024.0 if precision == "fp16" else 1.0
    sd = eg.leaves(_weights(case), torch.float32, DEV)
    keep = {}
    outs = _hip(case, precision, sd, keep)
    (_loss(case, outs, torch.float32, DEV) * scale).backward()
    got = {n: w.grad for n, w in sd.items()}
    assert all(g is not None for g in got.values())
    ref, tape, prefix = _f64_on(case, eg.hip_masks(keep), scale)
    zb = eg.normed_biases(ref, c["norm"], prefix)
    e_hip = eg.errors(got, ref, tape, zb, prefix)
    # the float64 run's own masks against the HIP masks
    own = eg.Tape()
    _restated(case, {n: w.double() for n, w in _weights(case).items()}, [x.double() for x in _inputs(case)], own)
    hm = eg.hip_masks(keep)
    agree = {n: float((own.masks[n] == hm[n]).double().mean()) for n in hm}
    # the yardstick: library calls on the GPU, its own masks
    ysd = eg.leaves(_weights(case), torch.float32, DEV)
    ytape = eg.Tape()
    xs = [x.float().to(DEV) for x in _inputs(case)]
    if precision == "fp32":
        youts = _restated(case, ysd, xs, ytape)
    else:
        with torch.autocast("cuda", dtype=AUTOCAST[precision]):
            youts = _restated(case, ysd, xs, ytape)
    (_loss(case, youts, torch.float32, DEV) * scale).backward()
    yref, ytape64, _ = _f64_on(case, {n: m.cpu() for n, m in ytape.masks.items()}, scale)
    e_yard = eg.errors({n: w.grad for n, w in ysd.items()}, yref, ytape64, zb, prefix)
    return e_hip, e_yard, agree


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_whole_encoder_gradients(case, precision):
    """Measured on the MI355X (largest over the parameter tensors, HIP / yardstick):
    A fp32 4.7e-6 / 7.2e-6, fp16 8.9e-3 / 1.5e-2, bf16 7.7e-2 / 1.35e-1; B fp32 6.5e-7 / 7.8e-7, fp16 1.25e-1 / 1.26e-1,
    bf16 1.11e-1 / 1.11e-1; C fp32 2.7e-6 / 2.3e-6, fp16 5.3e-3 / 8.5e-3, bf16 4.8e-2 / 5.6e-2.  Biases under an
    instance norm: HIP 4e-8 .. 7e-8, yardstick 7e-8 (fp32) .. 2.8e-3 (bf16).  Mask agreement (minimum over the ReLUs):
    fp32 1.0 in all cases; fp16 0.9983 / 0.9997 / 0.9985; bf16 0.9896 / 0.9979 / 0.9875.  Every figure is printed
    before the assertions."""
    e_hip, e_yard, agree = _run(case, precision)
    for n in e_hip:
        print(f"{case} {precision} {n}: hip {e_hip[n]:.3e} yardstick {e_yard[n]:.3e}")
    print(f"{case} {precision} mask agreement: min {min(agree.values()):.6f}")
    worst = max(e_hip, key=e_hip.get)
    print(f"{case} {precision} worst tensor: {worst} hip {e_hip[worst]:.3e} yardstick {e_yard[worst]:.3e}")
    if precision == "fp32":
        assert min(agree.values()) >= AGREE_MIN, agree
    bad = {}
    for n in e_hip:
        bound = 2 * e_yard[n] if precision != "fp32" else min(1e-4, max(1e-5, 2 * e_yard[n]))
        if not e_hip[n] <= bound:
            bad[n] = (e_hip[n], bound)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------
# per layer, through the torch.ops entries
# ---------------------------------------------------------------------------------------------------------------
WIDTHS = ((27, 8, 8), (27, 16, 16), (27, 24, 24), (1, 32, 8), (1, 8, 32), (1, 64, 24), (1, 96, 160))
VOL = (5, 6, 17)


@functools.lru_cache(maxsize=None)
def _layer_case(taps, cin, cout, stride, prologue):
    """Float32 inputs and the float64 F.conv3d autograd results on the CPU."""
    k = 3 if taps == 27 else 1
    seed = 7000 + 97 * cin + 13 * cout + 5 * stride + prologue + taps
    x = _rand(seed, (2, cin) + VOL).float()
    w = (_rand(seed + 1, (cout, cin, k, k, k)) * (cin * taps) ** -0.5).float()
    ss = torch.stack([_rand(seed + 2, (2, cin)) * 0.5 + 1.0, _rand(seed + 3, (2, cin)) * 0.3], dim=-1).float().contiguous()
    xd, wd = x.double(), w.double().requires_grad_(True)
    a = xd
    if prologue == 2:
        a = xd * ss[..., 0].double()[:, :, None, None, None] + ss[..., 1].double()[:, :, None, None, None]
    if prologue != 0:
        a = F.relu(a)
    a = a.detach().requires_grad_(True)
    y = F.conv3d(a, wd, None, stride=stride, padding=k // 2)
    g = _rand(seed + 4, y.shape).float()
    y.backward(g.double())
    return x, w, ss, g, wd.grad, a.grad


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("stride", (1, 2))
@pytest.mark.parametrize("taps,cin,cout", WIDTHS)
def test_layer_wgrad_dgrad(taps, cin, cout, stride, precision):
    import dvccorr  # noqa: F401
    O = torch.ops.dvccorr
    for prologue in (0, 1, 2):
        x, w, ss, g, dw_ref, da_ref = _layer_case(taps, cin, cout, stride, prologue)
        dw = O.enc_wgrad(x.to(DEV), ss.to(DEV) if prologue == 2 else None, prologue, g.to(DEV), taps, stride, DT[precision])
        e = _err(dw, dw_ref)
        print(f"wgrad taps {taps} {cin}->{cout} stride {stride} prologue {prologue} {precision}: {e:.3e}")
        assert e <= LAYER_TOL[precision]
    packed = O.enc_pack_dgrad(w.to(DEV), DT[precision])
    dx = O.enc_dgrad(g.to(DEV), packed, taps, stride, cin, list(VOL), DT[precision])
    e = _err(dx, da_ref)
    print(f"dgrad taps {taps} {cin}->{cout} stride {stride} {precision}: {e:.3e}")
    assert e <= LAYER_TOL[precision]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("stride", (1, 2))
def test_stem_wgrad(stride, precision):
    import dvccorr  # noqa: F401
    x = _rand(8100 + stride, (2, 1, 9, 6, 17)).float()
    w = torch.zeros(32, 1, 7, 7, 7, dtype=torch.float64, requires_grad=True)
    y = F.conv3d(x.double(), w, None, stride=stride, padding=3)
    g = _rand(8110 + stride, y.shape).float()
    y.backward(g.double())
    dw = torch.ops.dvccorr.enc_wgrad(x.to(DEV), None, 0, g.to(DEV), 343, stride, DT[precision])
    e = _err(dw, w.grad)
    print(f"stem wgrad stride {stride} {precision}: {e:.3e}")
    assert e <= LAYER_TOL[precision]


@pytest.mark.parametrize("mask", (False, True))
@pytest.mark.parametrize("normed", (False, True))
def test_norm_grad(normed, mask):
    """g_x and db against float64 autograd of instance_norm (+ ReLU) from the same float32 inputs, db normalised by
    the largest per-channel sum of |g_x|; the two per-plane means enter only through g_x.  C = 24 planes of
    9 x 30 x 17 voxels: two chunks per plane."""
    import dvccorr  # noqa: F401
    shape = (2, 24, 9, 30, 17)
    x = _rand(8200, shape).float()
    g = _rand(8201, shape).float()
    xd = x.double().requires_grad_(True)
    if normed:
        mean, var = xd.mean(dim=(2, 3, 4), keepdim=True), xd.var(dim=(2, 3, 4), unbiased=False, keepdim=True)
        a = 1.0 / torch.sqrt(var + 1e-5)
        ss = torch.stack([a.flatten(1), (-mean * a).flatten(1)], dim=-1).detach().float().contiguous()
        n = (xd - mean) * a
    else:
        ss, n = None, xd
    (F.relu(n) if mask else n).backward(g.double())
    if not normed and not mask:
        gx, db = torch.ops.dvccorr.enc_norm_grad(g.to(DEV), None, None, False, False, True)
        assert gx.numel() == 0
    else:
        gx, db = torch.ops.dvccorr.enc_norm_grad(g.to(DEV), x.to(DEV), None if ss is None else ss.to(DEV), mask, True, True)
        assert _err(gx, xd.grad) <= LAYER_TOL["fp32"]
    scale = float(xd.grad.abs().sum(dim=(0, 2, 3, 4)).max())
    e = float((db.double().cpu() - xd.grad.sum(dim=(0, 2, 3, 4))).abs().max()) / scale
    print(f"norm_grad normed {normed} mask {mask}: db {e:.3e}")
    assert e <= LAYER_TOL["fp32"]


# ---------------------------------------------------------------------------------------------------------------
# the entry points' contracts
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_forward_bit_identical(precision):
    import dvccorr
    for case in ("A", "B"):
        c = CASES[case]
        sd = {n: w.float().to(DEV) for n, w in _weights(case).items()}
        xs = [x.float().to(DEV) for x in _inputs(case)]
        with torch.no_grad():
            if c["ctx"]:
                ref = dvccorr.ContextEncoder(sd, c["kind"], c["norm"], HIDDEN, c["out"] - HIDDEN, precision)(xs[0])
            else:
                ref = dvccorr.Encoder(sd, c["kind"], c["norm"], precision)(xs)
        got = _hip(case, precision, {n: w.clone().requires_grad_(True) for n, w in sd.items()})
        assert len(got) == len(ref) and all(torch.equal(a, b) for a, b in zip(got, ref))


def _grads(case, precision, sd):
    for w in sd.values():
        w.grad = None
    _loss(case, _hip(case, precision, sd), torch.float32, DEV).backward()
    return {n: (None if w.grad is None else w.grad.clone()) for n, w in sd.items()}


def test_backward_bit_identical_and_selective():
    sd = eg.leaves(_weights("A"), torch.float32, DEV)
    g1, g2 = _grads("A", "fp32", sd), _grads("A", "fp32", sd)
    assert all(torch.equal(g1[n], g2[n]) for n in g1)
    frozen = {"conv1.weight", "layer2.0.conv2.bias", "layer2.0.downsample.0.weight", "conv2.weight"}
    part = {n: w.detach().clone().requires_grad_(n not in frozen) for n, w in sd.items()}
    g3 = _grads("A", "fp32", part)
    for n in g1:
        assert (g3[n] is None) if n in frozen else torch.equal(g3[n], g1[n]), n
    # only the last layers ask: everything upstream is skipped, the values stay.  The first layer that asks is a block
    # boundary, a conv3, a conv2, a conv1 next to a shortcut convolution, or only the shortcut convolution
    for first in (("layer3.1", "conv2."), ("layer3.1.conv3", "conv2."), ("layer3.1.conv2", "layer3.1.conv3"),
                  ("layer2.0.conv3",), ("layer2.0.conv2.bias",), ("layer3.0.conv1", "conv2.bias"),
                  ("layer3.0.downsample.0",), ("conv2.bias",)):
        tail = {n: w.detach().clone().requires_grad_(n.startswith(first)) for n, w in sd.items()}
        g4 = _grads("A", "fp32", tail)
        for n in g1:
            assert (g4[n] is None) if not tail[n].requires_grad else torch.equal(g4[n], g1[n]), (first, n)


def test_inplace_update_repacks():
    """After an in-place add_ on weights the next forward and backward use the new values (forward and dgrad packs)."""
    sd = eg.leaves(_weights("A"), torch.float32, DEV)
    _grads("A", "fp32", sd)
    with torch.no_grad():
        for n in ("layer2.0.conv2.weight", "layer3.0.downsample.0.weight", "conv2.weight"):
            sd[n].add_(0.05 * _rand(9000, sd[n].shape).to(DEV))
    cached = dict(sd["conv1.weight"]._dvc_ad_encoders)   # the weight set's own encoder objects (pack caches)
    got = _grads("A", "fp32", sd)
    assert all(sd["conv1.weight"]._dvc_ad_encoders[k] is v for k, v in cached.items()) and cached
    fresh = _grads("A", "fp32", {n: w.detach().clone().requires_grad_(True) for n, w in sd.items()})
    assert all(torch.equal(got[n], fresh[n]) for n in got)


def test_volume_grad_refused():
    import dvccorr
    sd = eg.leaves(_weights("C"), torch.float32, DEV)
    x = _inputs("C")[0].float().to(DEV).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="volume"):
        dvccorr.encoder_ad(x, sd, "1/1", "instance")


def test_uncovered_encoder_matches_autograd():
    """Group norm runs the library composition under autograd; it matches float64 autograd of an independent
    restatement (tests/encoder_grad.py) to 1e-5 per tensor, the affine norm parameters included."""
    import dvccorr
    sd = eg.leaves(_weights("C"), torch.float32, DEV)
    for n in list(sd):
        if n.endswith(".weight"):
            base, co = n[:-len("weight")], sd[n].shape[0]
            nn_ = "norm1." if base == "conv1." else base.replace("conv", "norm").replace("downsample.0", "norm4")
            if base != "conv2.":
                sd[nn_ + "weight"] = (1 + 0.1 * _rand(9100 + co, (co,))).float().to(DEV).requires_grad_(True)
                sd[nn_ + "bias"] = (0.1 * _rand(9200 + co, (co,))).float().to(DEV).requires_grad_(True)
    x = _inputs("C")[0].float().to(DEV)
    G = _rand(9300, (1, 128, 9, 6, 17)).float().to(DEV)
    (dvccorr.encoder_ad(x, sd, "1/1", "group") * G).sum().backward()
    # the reference: the harness's own F.conv3d / F.group_norm restatement in float64 on the CPU, plain autograd
    ref = eg.leaves(sd, torch.float64, "cpu")
    (eg.encoder(x.double().cpu(), ref, eg.STRIDES["1/1"], "group") * G.double().cpu()).sum().backward()
    assert any(n.startswith("norm1.") for n in ref) and all(w.grad is not None for w in ref.values())
    for n in sd:
        e = _err(sd[n].grad, ref[n].grad)
        print(f"group norm {n}: {e:.3e}")
        assert e <= 1e-5, n
