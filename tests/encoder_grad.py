"""Test-only float64 restatement of the feature and context encoders with a ReLU tape (TEST INFRASTRUCTURE, never
product code), for the gradient tests of dvccorr.encoder_ad / context_encoder_ad.

The restatement is functional: it runs from a state dict (the names of tests/raftdvc_encoder.py / the reference's
extractor.py) in the dtype and on the device of its tensors, for any (conv1, layer1, layer2, layer3) strides and norm
'instance', 'none' or 'group' (affine, channels // 8 groups; its weights under the reference's norm names).  A Tape,
like train_loop.Tape, either records `act > 0` of every ReLU (the stem's, three per block) or consumes a record: every ReLU becomes pre * mask, and the share of `pre > 0 == mask` is reported per ReLU.
With a consumed record the function is smooth around the recorded point, so its gradients are those of the run that
produced the masks.  The tape also keeps every raw convolution output (with its gradient retained), from which the
tests take the scale of a bias gradient that cancels under an instance norm.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

import prng

BLOCKS = tuple(f"layer{i}.{j}" for i in (1, 2, 3) for j in (0, 1))
STRIDES = {"1/8": (2, 1, 2, 2), "1/4": (2, 1, 2, 1), "1/2": (2, 1, 1, 1), "1/1": (1, 1, 1, 1)}
EPS = 1e-5


class Tape:
    def __init__(self, masks=None):
        self.recording = masks is None
        self.masks = {} if masks is None else masks
        self.agree = {}
        self.raw = {}

    def relu(self, name, pre):
        if self.recording:
            self.masks[name] = (pre > 0).detach()
            return F.relu(pre)
        m = self.masks[name].to(pre.device)
        self.agree[name] = float(((pre > 0) == m).double().mean())
        return pre * m.to(pre.dtype)


def _relu(tape, name, pre):
    return F.relu(pre) if tape is None else tape.relu(name, pre)


def encoder(x, sd, strides, norm="instance", tape=None, prefix=""):
    """conv2's raw output.  sd: name -> tensor (weights may require grad)."""
    def conv(name, t, stride, pad):
        y = F.conv3d(t, sd[prefix + name + ".weight"], sd[prefix + name + ".bias"], stride=stride, padding=pad)
        if tape is not None:
            if y.requires_grad:
                y.retain_grad()
            tape.raw[name] = y
        return y

    def nrm(t, name):
        if norm == "group":   # extractor.py: GroupNorm(num_groups = channels // 8), affine
            return F.group_norm(t, max(1, t.shape[1] // 8), sd[prefix + name + ".weight"], sd[prefix + name + ".bias"], EPS)
        return F.instance_norm(t, eps=EPS) if norm == "instance" else t

    x = _relu(tape, "conv1", nrm(conv("conv1", x, strides[0], 3), "norm1"))
    for blk in BLOCKS:
        stride = strides[int(blk[5])] if blk.endswith(".0") else 1
        y = _relu(tape, blk + ".relu1", nrm(conv(blk + ".conv1", x, 1, 0), blk + ".norm1"))
        y = _relu(tape, blk + ".relu2", nrm(conv(blk + ".conv2", y, stride, 1), blk + ".norm2"))
        y = nrm(conv(blk + ".conv3", y, 1, 0), blk + ".norm3")
        r = nrm(conv(blk + ".downsample.0", x, stride, 0), blk + ".norm4") \
            if prefix + blk + ".downsample.0.weight" in sd else x
        x = _relu(tape, blk + ".out", y + r)
    return conv("conv2", x, 1, 0)


def context_encoder(x, sd, strides, hidden, norm="none", tape=None, prefix="encoder."):
    y = encoder(x, sd, strides, norm, tape, prefix)
    return torch.tanh(y[:, :hidden]), F.relu(y[:, hidden:])


def make_weights(strides, output_dim, seed0, prefix="", dtype=torch.float64):
    """A state dict of the encoder's forty-odd convolution tensors, uniform(-b, b), b = 1 / sqrt(fan_in)."""
    shapes = {"conv1": (32, 1, 7)}
    cin = 32
    for k, blk in enumerate(BLOCKS):
        planes = (32, 64, 96)[k // 2]
        stride = strides[1 + k // 2] if k % 2 == 0 else 1
        shapes[blk + ".conv1"] = (planes // 4, cin, 1)
        shapes[blk + ".conv2"] = (planes // 4, planes // 4, 3)
        shapes[blk + ".conv3"] = (planes, planes // 4, 1)
        if stride != 1 or cin != planes:
            shapes[blk + ".downsample.0"] = (planes, cin, 1)
        cin = planes
    shapes["conv2"] = (output_dim, cin, 1)
    sd = {}
    for i, (n, (co, ci, k)) in enumerate(shapes.items()):
        b = (ci * k ** 3) ** -0.5
        sd[prefix + n + ".weight"] = torch.from_numpy(prng.uniform(seed0 + 2 * i, (co, ci, k, k, k), -b, b)).to(dtype)
        sd[prefix + n + ".bias"] = torch.from_numpy(prng.uniform(seed0 + 2 * i + 1, (co,), -b, b)).to(dtype)
    return sd


def leaves(sd, dtype, device):
    """Independent leaf copies of a state dict that require grad."""
    return {n: w.detach().to(device=device, dtype=dtype).clone().requires_grad_(True) for n, w in sd.items()}


def hip_masks(keep):
    """The ReLU masks of a HIP run from the tensors encoder_ad kept (its `keep` hook): the sign of the float32 fused
    multiply-add x a + s of the forward's prologue, evaluated exactly in float64 (the product of two float32 values
    and the sum are exact enough in double that the sign is the fma's), or of x itself without a norm; `out > 0` for
    the block outputs."""
    def of(layer):
        x = keep[layer].double()
        ss = keep.get(layer + ".ss")
        if ss is None:
            return (x > 0).cpu()
        a, s = ss[..., 0].double(), ss[..., 1].double()
        return (x * a[:, :, None, None, None] + s[:, :, None, None, None] > 0).cpu()

    masks = {"conv1": of("conv1")}
    for blk in BLOCKS:
        masks[blk + ".relu1"] = of(blk + ".conv1")
        masks[blk + ".relu2"] = of(blk + ".conv2")
        masks[blk + ".out"] = (keep[blk + ".out"] > 0).cpu()
    return masks


def normed_biases(sd, norm, prefix=""):
    """Names of the biases whose convolution feeds an instance norm: their gradient is exactly zero."""
    if norm != "instance":
        return set()
    return {n for n in sd if n.endswith(".bias") and n != prefix + "conv2.bias"}


def errors(got, ref, tape, zero_biases, prefix=""):
    """Per parameter: max |got - ref| / max |ref|; for a bias under an instance norm, / max_c sum_{b, v} |g_x| of the
    float64 run (the scale of the sum that cancels)."""
    out = {}
    for n, r in ref.items():
        g = got[n].detach().double().cpu()
        r = r.detach().double().cpu()
        if n in zero_biases:
            gx = tape.raw[n[len(prefix):-len(".bias")]].grad
            scale = float(gx.abs().sum(dim=(0, 2, 3, 4)).max())
        else:
            scale = float(r.abs().max())
        out[n] = float((g - r).abs().max()) / scale
    return out
