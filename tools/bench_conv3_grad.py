#!/usr/bin/env python3
"""Time the backward of the update block's four 3 x 3 x 3 layer shapes at (1, ., 32, 32, 32): the HIP backward of
dvccorr::conv3_ad (k_conv3_grad_prep + k_conv3_mfma on the transposed weights + k_conv3_wgrad, one timed region, and
each part alone) against the library's backward of the same layer (torch.autograd.grad through F.conv3d (+ ReLU)), in
fp32 and in fp16 (the library under torch.autocast), all in one process.

    python tools/bench_conv3_grad.py [--reps 30] [--warmup 5] [--out profiles/r09/conv3_grad_bench.json]

The protocol is tools/bench_update.py's: every repetition is timed with a pair of device events and all paths alternate
inside each repetition.  Both sides compute the input, weight and bias gradients of every layer.  The errors of dW and
dx (max-normalised, fp32 / fp16 / bf16) are against F.conv3d in float64 on the GPU with the ReLU mask of the HIP
forward's own output."""
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

# layer, input channels (two sources for encoder.conv), ReLU
LAYERS = (("encoder.convf2", (64,), True), ("encoder.conv", (96, 32), True), ("flow_head.conv1", (96,), True),
          ("flow_head.conv2", (128,), False))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "conv3_grad_bench.json"))
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("at least 20 timed repetitions")
    import dvccorr  # noqa: F401
    from dvccorr import ops
    import prng
    import raftdvc_loop as rl
    dev = torch.device("cuda:0")
    S = a.size
    vol = (S, S, S)
    p = rl.load_params(dev)
    paths, flops, errs = {}, {}, {}
    seed = 9400

    def nerr(v, ref):
        return float((v.double() - ref).abs().max() / ref.abs().max())
    for layer, cins, relu in LAYERS:
        w, b = p[layer + ".weight"], p[layer + ".bias"]
        cout, cin = int(w.shape[0]), sum(cins)
        srcs = []
        for c in cins:
            srcs.append(torch.relu(torch.from_numpy(prng.normal(seed, (1, c, *vol)))).to(dev))
            seed += 1
        gy = torch.from_numpy(prng.uniform(seed, (1, cout, *vol), -1.0, 1.0)).to(dev)
        seed += 1
        x0, x1 = srcs[0], (srcs[1] if len(srcs) > 1 else None)
        xcat = x0 if x1 is None else torch.cat(srcs, dim=1)
        flops[layer] = 2 * 2 * S ** 3 * 27 * cin * cout   # dgrad + wgrad

        # the library's backward: the graph is built once, every repetition differentiates it
        def graph(half, xcat=xcat, w=w, b=b, relu=relu):
            xs, ws, bs = (t.detach().clone().requires_grad_(True) for t in (xcat, w, b))
            with torch.autocast("cuda", dtype=torch.float16, enabled=half):
                y = F.conv3d(xs, ws, bs, padding=1)
                y = F.relu(y) if relu else y
            return y, (xs, ws, bs)
        for name, half in (("torch_fp32", False), ("torch_fp16", True)):
            y, leaves = graph(half)
            paths[f"{layer}/{name}"] = lambda y=y, leaves=leaves, gy=gy: torch.autograd.grad(
                y, leaves, gy.to(y.dtype), retain_graph=True)

        for prec in ("fp32", "fp16", "bf16"):
            dtype = ops.dtype_code(prec)
            y = torch.empty((1, cout, *vol), device=dev)
            ops.conv3(x0, x1, ops.conv3_pack(w, b, dtype), y, 0, cout, relu, dtype)
            pk_d = ops.conv3_pack_dgrad(w, dtype)
            dcat = torch.empty((1, cin, *vol), device=dev)
            yk = y if relu else None

            def prep(gy=gy, yk=yk, relu=relu):
                return ops.conv3_grad_prep(gy, yk, relu)
            g = prep()[0]

            def dgrad(g=g, pk_d=pk_d, dcat=dcat, cin=cin, dtype=dtype):
                return ops.conv3(g, None, pk_d, dcat, 0, cin, False, dtype)

            def wgrad(g=g, x0=x0, x1=x1, dtype=dtype):
                return ops.conv3_wgrad(x0, x1, g, dtype)

            def backward(prep=prep, x0=x0, x1=x1, pk_d=pk_d, dcat=dcat, cin=cin, dtype=dtype):
                gg, db = prep()
                dw = ops.conv3_wgrad(x0, x1, gg, dtype)
                ops.conv3(gg, None, pk_d, dcat, 0, cin, False, dtype)
                return dcat, dw, db
            # errors against float64 on the GPU, the mask from this precision's own forward
            xs, ws = xcat.double().requires_grad_(True), w.double().requires_grad_(True)
            rx, rw = torch.autograd.grad(F.conv3d(xs, ws, b.double(), padding=1), (xs, ws), g.double())
            dx, dw, _ = backward()
            errs[f"{layer}/{prec}"] = {"dx": nerr(dx, rx), "dw": nerr(dw, rw)}
            del xs, ws, rx, rw
            if prec != "bf16":
                paths[f"{layer}/hip_{prec}"] = backward
                paths[f"{layer}/hip_{prec}_prep"], paths[f"{layer}/hip_{prec}_dgrad"] = prep, dgrad
                paths[f"{layer}/hip_{prec}_wgrad"] = wgrad

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
           "flop": flops, "errors_vs_float64": errs, "paths": {}}
    for k, t in times.items():
        med = statistics.median(t)
        res["paths"][k] = {"median_ms": med, "min_ms": min(t), "max_ms": max(t),
                           "tflops": flops[k.split("/")[0]] / med / 1e9}
    res["layers_sum"] = {}
    for prec in ("fp32", "fp16"):
        hip = sum(res["paths"][f"{l[0]}/hip_{prec}"]["median_ms"] for l in LAYERS)
        lib_min = sum(res["paths"][f"{l[0]}/torch_{prec}"]["min_ms"] for l in LAYERS)
        res["layers_sum"][prec] = {"hip_median_ms": hip, "torch_min_ms": lib_min,
                                   "hip_median_below_torch_min": hip < lib_min}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
