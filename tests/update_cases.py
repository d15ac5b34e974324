"""Test-only helpers of the UpdateBlock tests: fixture inputs, parameters and the per-layer CPU checker (built on
raftdvc_loop._conv)."""
from __future__ import annotations

import functools
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

import prng
import raftdvc_loop as rl
from conftest import GOLDEN, load_golden

CASES = ("upd_888", "upd_b2_597", "upd_215")
# layer -> (stored input(s), stored output, padding, relu); inputs are concatenated along the channels
LAYERS = {
    "encoder.convf1": (("flow",), "flo1", 3, True),
    "encoder.convf2": (("flo1",), "flo2", 1, True),
    "encoder.conv": (("cor", "flo2"), "motion", 1, True),
    "flow_head.conv1": (("net",), "hid", 1, True),
    "flow_head.conv2": (("hid",), "delta_flow", 1, False),
    "uncertainty_head.conv1": (("net",), "unc_hid", 1, True),
    "uncertainty_head.conv2": (("unc_hid",), "log_b", 1, False),
}


@functools.lru_cache(maxsize=None)
def _meta():
    with open(os.path.join(GOLDEN, "update_meta.json")) as f:
        return json.load(f)


def case_meta(name):
    for n, B, vol, mode, seeds in _meta()["cases"]:
        if n == name:
            return B, tuple(vol), mode, tuple(seeds)
    raise KeyError(name)


def params(name="upd_888"):
    """BasicUpdateBlock.state_dict() names -> float32 CPU tensors of the case's block (epe_meta.json's parameters, plus
    update_meta.json's uncertainty head where the case has one)."""
    p = rl.load_params("cpu")
    mode = case_meta(name)[2]
    for n, shape, seed, b in _meta()["uncertainty_params"].get(mode, []):
        p[n] = torch.from_numpy(prng.uniform(seed, tuple(shape), -b, b))
    return p


@functools.lru_cache(maxsize=None)
def _case(name):
    B, vol, mode, (sn, sc, sf, sr) = case_meta(name)
    net = prng.uniform(sn, (B, 96) + vol, -1.0, 1.0)
    context = np.maximum(prng.normal(sc, (B, 64) + vol), 0.0).astype(np.float32)
    flow = prng.uniform(sf, (B, 3) + vol, -2.0, 2.0)
    corr = (0.5 * prng.normal(sr, (B, 2916) + vol)).astype(np.float32)
    ref = dict(load_golden(name + "_enc.npz"))
    ref.update(load_golden(name + "_head.npz"))
    assert tuple(int(v) for v in ref["shape"]) == (B,) + vol
    out = {k: torch.from_numpy(v) for k, v in ref.items() if k not in ("shape", "seeds")}
    out["motion"] = out["motion_features"][:, :80].contiguous()
    out.update(net0=torch.from_numpy(net), context=torch.from_numpy(context), flow=torch.from_numpy(flow),
               corr=torch.from_numpy(corr))
    return out


def case(name):
    """Inputs (net0, context, flow, corr) and the reference's stored activations of one fixture, as CPU tensors that
    callers must not modify (they are shared)."""
    return _case(name)


def layers_of(name):
    return [l for l in LAYERS if not l.startswith("uncertainty") or case_meta(name)[2] != "none"]


def layer_inputs(c, layer):
    """The stored input tensors of a layer ('net' is the GRU's output, the heads' input)."""
    return [c[k] for k in LAYERS[layer][0]]


def check_layer(p, layer, *srcs):
    """One layer on the CPU through raftdvc_loop._conv."""
    _, _, pad, relu = LAYERS[layer]
    y = rl._conv(p, layer, srcs[0] if len(srcs) == 1 else torch.cat(srcs, dim=1), pad)
    return F.relu(y) if relu else y


def conv_ref(x, weight, bias, relu=False, x2=None):
    """F.conv3d of cat[x, x2] with 'same' padding through raftdvc_loop._conv, for synthetic layers."""
    y = rl._conv({"l.weight": weight, "l.bias": bias}, "l", x if x2 is None else torch.cat([x, x2], dim=1),
                 weight.shape[2] // 2)
    return F.relu(y) if relu else y


def checker(p, net, context, flow, cor=None, corr=None):
    """BasicUpdateBlock.forward on the CPU: (net, delta_flow, log_b)."""
    net, delta = rl.update_block(p, net, context, flow, corr=corr, cor=cor)
    log_b = None
    if "uncertainty_head.conv1.weight" in p:
        log_b = check_layer(p, "uncertainty_head.conv2", check_layer(p, "uncertainty_head.conv1", net))
    return net, delta, log_b


def err(a, ref) -> float:
    """Max-normalised error."""
    a, ref = torch.as_tensor(a).double().cpu(), torch.as_tensor(ref).double().cpu()
    return float((a - ref).abs().max() / ref.abs().max())
