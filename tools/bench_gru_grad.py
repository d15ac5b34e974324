#!/usr/bin/env python3
"""Time the update block's GRU in training at (1, 96 | 147, 32, 32, 32): the HIP training forward (k_sep_gru_pass with
SAVE) and backward of dvccorr::sep_gru_ad (and the backward's parts: prep, dgrad, wgrad, over the three passes) against
the same GRU as the library composition (nine F.conv3d calls) with torch.autograd.grad for dh, dx and the eighteen
parameter gradients, in fp32 and in fp16 (the library under torch.autocast), all in one process.  The inference
forward is timed beside the training forward: the difference is the cost of the saves.

    python tools/bench_gru_grad.py [--reps 30] [--warmup 5] [--out profiles/r10/gru_grad_bench.json]

The protocol is tools/bench_conv3_grad.py's: every repetition is timed with a pair of device events and all paths
alternate inside each repetition.  The condition: the HIP median of training forward + backward is below the library's
minimum of forward + backward, in both precisions."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "raft-dvc_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

_AXES = (("h", (2, 0, 0)), ("w", (0, 2, 0)), ("d", (0, 0, 2)))


def composition(p, h, x):
    for ax, pad in _AXES:
        hx = torch.cat([h, x], dim=1)
        z = torch.sigmoid(F.conv3d(hx, p[f"convz_{ax}.weight"], p[f"convz_{ax}.bias"], padding=pad))
        r = torch.sigmoid(F.conv3d(hx, p[f"convr_{ax}.weight"], p[f"convr_{ax}.bias"], padding=pad))
        q = torch.tanh(F.conv3d(torch.cat([r * h, x], dim=1), p[f"convq_{ax}.weight"], p[f"convq_{ax}.bias"],
                                padding=pad))
        h = (1 - z) * h + z * q
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "gru_grad_bench.json"))
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("at least 20 timed repetitions")
    import dvccorr
    from dvccorr import ops
    import gru_cases
    import prng
    dev = torch.device("cuda:0")
    S = a.size
    vol = (S, S, S)
    p = {n: t.to(dev) for n, t in gru_cases.params().items()}
    names = dvccorr.update.GRU_WEIGHT_NAMES
    h = torch.from_numpy(prng.uniform(9700, (1, 96, *vol), -1.0, 1.0)).to(dev)
    x = torch.from_numpy(prng.normal(9701, (1, 147, *vol))).to(dev)
    gy = torch.from_numpy(prng.uniform(9702, (1, 96, *vol), -1.0, 1.0)).to(dev)
    paths = {}

    for name, half in (("torch_fp32", False), ("torch_fp16", True)):
        def fwd(half=half):
            leaves = [t.detach().clone().requires_grad_(True) for t in [h, x] + [p[n] for n in names]]
            with torch.autocast("cuda", dtype=torch.float16, enabled=half):
                y = composition(dict(zip(names, leaves[2:])), leaves[0], leaves[1])
            return y, leaves
        y, leaves = fwd()
        paths[f"{name}_forward"] = fwd
        paths[f"{name}_backward"] = lambda y=y, leaves=leaves: torch.autograd.grad(y, leaves, gy.to(y.dtype),
                                                                                   retain_graph=True)

    for prec in ("fp32", "fp16"):
        dtype = ops.dtype_code(prec)
        packed, packed_d = ops.gru_pack(p, dtype), ops.gru_pack_dgrad(p, dtype)
        _, saved = ops.sep_gru_save(h, x, packed, dtype)
        dx = torch.empty_like(x)
        z, r, q, h_in = saved[6], saved[7], saved[8], saved[10]
        aq, az, dh, _, _ = ops.gru_grad_prep(gy, z, q, h_in)
        ar, _ = ops.sep_gru_dgrad(aq, az, h_in, r, packed_d[2], dh.clone(), dx, 2, False, dtype)

        def backward(dtype=dtype, packed_d=packed_d, saved=saved, dx=dx):
            g, out = gy, []
            for ax in (2, 1, 0):
                hh = (h, saved[9], saved[10])[ax]
                zz, rr, qq = saved[3 * ax], saved[3 * ax + 1], saved[3 * ax + 2]
                aq_, az_, dh_, dbq, dbz = ops.gru_grad_prep(g, zz, qq, hh)
                ar_, dbr = ops.sep_gru_dgrad(aq_, az_, hh, rr, packed_d[ax], dh_, dx, ax, ax != 2, dtype)
                out.append((ops.gru_wgrad(hh, x, rr, az_, ar_, aq_, ax, dtype), dbq, dbz, dbr))
                g = dh_
            return g, dx, out
        paths[f"hip_{prec}_forward_inference"] = lambda packed=packed, dtype=dtype: ops.sep_gru(h, x, packed, dtype)
        paths[f"hip_{prec}_forward"] = lambda packed=packed, dtype=dtype: ops.sep_gru_save(h, x, packed, dtype)
        paths[f"hip_{prec}_backward"] = backward
        # the parts, three passes' worth each (the d pass's operands stand in for all three)
        paths[f"hip_{prec}_prep"] = lambda z=z, q=q, h_in=h_in: [ops.gru_grad_prep(gy, z, q, h_in) for _ in range(3)]
        paths[f"hip_{prec}_dgrad"] = lambda aq=aq, az=az, h_in=h_in, r=r, packed_d=packed_d, dh=dh, dx=dx, dtype=dtype: [
            ops.sep_gru_dgrad(aq, az, h_in, r, packed_d[ax], dh, dx, ax, True, dtype) for ax in range(3)]
        paths[f"hip_{prec}_wgrad"] = lambda aq=aq, az=az, ar=ar, h_in=h_in, r=r, dtype=dtype: [
            ops.gru_wgrad(h_in, x, r, az, ar, aq, ax, dtype) for ax in range(3)]

    times = {k: [] for k in paths}
    for _ in range(a.warmup):
        for f in paths.values():
            f()
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for k, f in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    res = {"shape": [1, S, S, S], "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "paths": {k: {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)}
                     for k, t in times.items()}, "training": {}}
    for prec in ("fp32", "fp16"):
        hip = res["paths"][f"hip_{prec}_forward"]["median_ms"] + res["paths"][f"hip_{prec}_backward"]["median_ms"]
        lib = res["paths"][f"torch_{prec}_forward"]["min_ms"] + res["paths"][f"torch_{prec}_backward"]["min_ms"]
        res["training"][prec] = {"hip_median_ms": hip, "torch_min_ms": lib, "hip_median_below_torch_min": hip < lib}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
