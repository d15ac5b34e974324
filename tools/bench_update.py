#!/usr/bin/env python3
"""Time the update block's plain convolutions and the whole block at config #3's low-resolution shape,
(1, ., 32, 32, 32): every layer on HIP (k_conv7_flow / k_conv3_mfma) against that layer's F.conv3d (+ ReLU), in fp32
and in fp16 (the library under torch.autocast), and the whole dvccorr.UpdateBlock call against
tests/raftdvc_loop.update_block (the library composition) and against that composition with the GRU swapped for
dvccorr.SepConvGRU, all in one process.

    python tools/bench_update.py [--reps 30] [--warmup 5] [--out profiles/r08/update_bench.json]

Every repetition is timed with a pair of device events; all paths alternate inside each repetition.  FLOP are
counted from the layer shapes (2 * voxels * taps * cin * cout); "mfma_share" is that count over the median time over
the chip's dense bf16 MFMA peak (2.5 PFLOP/s; the fp32 path issues three MFMAs per product).  "issued_ratio" is the
MFMA work k_conv3_mfma issues over the layer's: input channels padded to 32, output channels to the instance's tiles
(1, 2, 4, 5 or 8 of 16) and the volume to whole 4 x 4 x 16 boxes."""
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

BF16_PEAK = 2.5e15
# layer, input channels (two sources for encoder.conv), kernel size, ReLU
LAYERS = (("encoder.convf1", (3,), 7, True), ("encoder.convf2", (64,), 3, True), ("encoder.conv", (96, 32), 3, True),
          ("flow_head.conv1", (96,), 3, True), ("flow_head.conv2", (128,), 3, False))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "update_bench.json"))
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("at least 20 timed repetitions")
    import dvccorr
    from dvccorr import _lib, ops
    import prng
    import raftdvc_loop as rl
    dev = torch.device("cuda:0")
    S = a.size
    vol = (S, S, S)
    p = rl.load_params(dev)
    paths, flops, issued = {}, {}, {}

    def boxes(t):
        return -(-S // t) * t
    padded_vox = boxes(_lib.CONV3_TH) * boxes(_lib.CONV3_TW) * boxes(_lib.CONV3_TD)
    seed = 9200
    for layer, cins, k, relu in LAYERS:
        w, b = p[layer + ".weight"], p[layer + ".bias"]
        cout = int(w.shape[0])
        srcs = []
        for c in cins:
            srcs.append(torch.relu(torch.from_numpy(prng.normal(seed, (1, c, *vol)))).to(dev))
            seed += 1
        x = srcs[0] if len(srcs) == 1 else torch.cat(srcs, dim=1)
        flops[layer] = 2 * S ** 3 * k ** 3 * sum(cins) * cout
        if k == 3:
            tiles = ops.lib().dvc_conv3_packed_bytes(1, cout, _lib.DVC_BF16) // (27 * 1024)
            issued[layer] = (padded_vox * -(-sum(cins) // 32) * 32 * tiles * 16) / (S ** 3 * sum(cins) * cout)

        def torch32(x=x, w=w, b=b, k=k, relu=relu):
            y = F.conv3d(x, w, b, padding=k // 2)
            return F.relu(y) if relu else y

        def torch16(f=torch32):
            with torch.autocast("cuda", dtype=torch.float16):
                return f()
        paths[layer + "/torch_fp32"], paths[layer + "/torch_fp16"] = torch32, torch16
        for prec in ("fp32", "fp16"):
            dtype = ops.dtype_code(prec)
            dst = torch.empty((1, cout, *vol), device=dev)
            if k == 7:
                packed = ops.conv7_flow_pack(w, b, dtype)
                paths[f"{layer}/hip_{prec}"] = lambda s=srcs, pk=packed, d=dst, t=dtype: ops.conv7_flow(s[0], pk, d, t)
            else:
                packed = ops.conv3_pack(w, b, dtype)
                s1 = srcs[1] if len(srcs) > 1 else None
                paths[f"{layer}/hip_{prec}"] = lambda s=srcs, s1=s1, pk=packed, d=dst, t=dtype, c=cout, r=relu: \
                    ops.conv3(s[0], s1, pk, d, 0, c, r, t)

    net = torch.from_numpy(prng.uniform(9301, (1, 96, *vol), -1.0, 1.0)).to(dev)
    ctx = torch.relu(torch.from_numpy(prng.normal(9302, (1, 64, *vol)))).to(dev)
    flow = torch.from_numpy(prng.uniform(9303, (1, 3, *vol), -2.0, 2.0)).to(dev)
    cor = torch.relu(torch.from_numpy(prng.normal(9304, (1, 96, *vol)))).to(dev)
    gw = {n[4:]: t for n, t in p.items() if n.startswith("gru.")}
    for prec in ("fp32", "fp16"):
        blk, gru = dvccorr.UpdateBlock(p, precision=prec), dvccorr.SepConvGRU(gw, precision=prec)
        paths[f"block/hip_{prec}"] = lambda blk=blk: blk(net, ctx, flow, cor=cor)

        def comp(prec=prec):
            if prec == "fp16":
                with torch.autocast("cuda", dtype=torch.float16):
                    return rl.update_block(p, net, ctx, flow, cor=cor)
            return rl.update_block(p, net, ctx, flow, cor=cor)

        def comp_hip_gru(prec=prec, gru=gru):
            def run():
                inp = torch.cat([ctx, rl.motion_features(p, flow, cor=cor)], dim=1)
                n = gru(net, inp.float())
                return n, rl._conv(p, "flow_head.conv2", F.relu(rl._conv(p, "flow_head.conv1", n, 1)), 1)
            if prec == "fp16":
                with torch.autocast("cuda", dtype=torch.float16):
                    return run()
            return run()
        paths[f"block/torch_{prec}"], paths[f"block/torch_hipgru_{prec}"] = comp, comp_hip_gru
    gru_flop = 9 * 2 * S ** 3 * 5 * 243 * 96
    flops["block"] = sum(flops[l[0]] for l in LAYERS) + gru_flop

    def first(v):
        return (v[1] if isinstance(v, tuple) else v).float()
    times = {k: [] for k in paths}
    with torch.no_grad():
        outs = {k: first(f()).clone() for k, f in paths.items()}
        err = {}
        for k, v in outs.items():
            ref = outs[k.split("/")[0] + "/torch_fp32"]
            err[k] = float((v - ref).abs().max() / ref.abs().max())
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
           "flop": flops, "issued_ratio": issued, "paths": {}}
    for k, t in times.items():
        med, flop = statistics.median(t), flops[k.split("/")[0]]
        res["paths"][k] = {"median_ms": med, "min_ms": min(t), "max_ms": max(t), "tflops": flop / med / 1e9,
                           "mfma_share": flop / (med * 1e-3) / BF16_PEAK, "err_vs_torch_fp32": err[k]}
    res["layers_sum"] = {}
    for prec in ("fp32", "fp16"):
        hip = sum(res["paths"][f"{l[0]}/hip_{prec}"]["median_ms"] for l in LAYERS)
        lib_min = sum(res["paths"][f"{l[0]}/torch_{prec}"]["min_ms"] for l in LAYERS)
        res["layers_sum"][prec] = {"hip_median_ms": hip, "torch_min_ms": lib_min, "hip_median_below_torch_min": hip < lib_min}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
