"""Test-only helpers of the SepConvGRU tests: fixture inputs, parameters and the per-pass CPU checker."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

import prng
import raftdvc_loop as rl
from conftest import GOLDEN, load_golden

CASES = ("gru_888", "gru_b2_597", "gru_215")
AXES = ("h", "w", "d")


def params(hidden=96, inp=147, seed0=None):
    """{'convz_h.weight': ...} float32 CPU tensors: the fixture's parameters (gru_meta.json seeds), or for other
    channel counts / seeds the same rule, uniform(-b, b) with b = 1/sqrt(fan_in)."""
    if (hidden, inp) == (96, 147) and seed0 is None:
        with open(os.path.join(GOLDEN, "gru_meta.json")) as f:
            meta = json.load(f)["params"]
        return {n: torch.from_numpy(prng.uniform(s, tuple(shape), -b, b)) for n, shape, s, b in meta}
    out, seed, b = {}, seed0 or 7500, (5 * (hidden + inp)) ** -0.5
    for a, ax in enumerate(AXES):
        for g in "zrq":
            k = [1, 1, 1]
            k[a] = 5
            out[f"conv{g}_{ax}.weight"] = torch.from_numpy(prng.uniform(seed, (hidden, hidden + inp, *k), -b, b))
            out[f"conv{g}_{ax}.bias"] = torch.from_numpy(prng.uniform(seed + 1, (hidden,), -b, b))
            seed += 2
    return out


def inputs(name):
    g = load_golden(name + ".npz")
    B, hid, inp, H, W, D = (int(v) for v in g["shape"])
    sh, sx = (int(v) for v in g["seeds"])
    h = torch.from_numpy(prng.uniform(sh, (B, hid, H, W, D), -1.0, 1.0))
    x = torch.from_numpy(prng.normal(sx, (B, inp, H, W, D)))
    return h, x, [torch.from_numpy(g[f"h_after_{ax}"]) for ax in AXES]


def checker_passes(p, h, x):
    """raftdvc_loop.sep_gru's hidden state after each pass (it is that function restricted to one axis at a time)."""
    out = []
    for ax in AXES:
        one = {f"gru.conv{g}_{a}.{k}": (p[f"conv{g}_{ax}.{k}"] if a == ax else None)
               for g in "zrq" for a in AXES for k in ("weight", "bias")}
        h = _one_pass(one, h, x, ax)
        out.append(h)
    return out


def _one_pass(one, h, x, ax):
    import torch.nn.functional as F
    pad = {"h": (2, 0, 0), "w": (0, 2, 0), "d": (0, 0, 2)}[ax]
    hx = torch.cat([h, x], dim=1)
    z = torch.sigmoid(F.conv3d(hx, one[f"gru.convz_{ax}.weight"], one[f"gru.convz_{ax}.bias"], padding=pad))
    r = torch.sigmoid(F.conv3d(hx, one[f"gru.convr_{ax}.weight"], one[f"gru.convr_{ax}.bias"], padding=pad))
    q = torch.tanh(F.conv3d(torch.cat([r * h, x], dim=1), one[f"gru.convq_{ax}.weight"],
                            one[f"gru.convq_{ax}.bias"], padding=pad))
    return (1 - z) * h + z * q


def checker(p, h, x):
    """raftdvc_loop.sep_gru with this module's parameter names."""
    return rl.sep_gru({"gru." + n: t for n, t in p.items()}, h, x)


def err(a, ref) -> float:
    """Max-normalised error."""
    a, ref = torch.as_tensor(a).double().cpu(), torch.as_tensor(ref).double().cpu()
    return float((a - ref).abs().max() / ref.abs().max())
