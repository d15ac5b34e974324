#!/usr/bin/env python3
"""Time the SepConvGRU forward at config #3's low-resolution shape, (1, 96 + 147, 32, 32, 32): the HIP GRU
(dvccorr.SepConvGRU, three k_sep_gru_pass launches) against the torch composition of the same math
(tests/raftdvc_loop.sep_gru: nine Conv3d, six cat and the elementwise ops -- what the package offered before), in fp32
and in fp16 (the composition under torch.autocast), all in one process.

    python tools/bench_gru.py [--reps 30] [--warmup 5] [--out profiles/r07/gru_bench.json]

Every repetition is timed with a pair of device events; the four paths alternate inside each repetition.  FLOP are
counted from the layer shapes (2 * voxels * 5 taps * 243 input channels * 96 outputs per convolution, nine
convolutions) and "mfma_share" is that count over the median time over the chip's dense bf16 MFMA peak (2.5 PFLOP/s;
the fp32 path issues three MFMAs per product, so its share of the issued work is three times the figure)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "raft-dvc_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

BF16_PEAK = 2.5e15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "gru_bench.json"))
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("at least 20 timed repetitions")
    import dvccorr
    import prng
    import raftdvc_loop as rl
    dev = torch.device("cuda:0")
    S, hid, inp = a.size, 96, 147
    b = (5 * (hid + inp)) ** -0.5
    w, seed = {}, 9000
    for ax, axis in zip("hwd", range(3)):
        for g in "zrq":
            k = [1, 1, 1]
            k[axis] = 5
            w[f"conv{g}_{ax}.weight"] = torch.from_numpy(prng.uniform(seed, (hid, hid + inp, *k), -b, b)).to(dev)
            w[f"conv{g}_{ax}.bias"] = torch.from_numpy(prng.uniform(seed + 1, (hid,), -b, b)).to(dev)
            seed += 2
    h = torch.from_numpy(prng.uniform(9100, (1, hid, S, S, S), -1.0, 1.0)).to(dev)
    x = torch.from_numpy(prng.normal(9101, (1, inp, S, S, S))).to(dev)
    p = {"gru." + n: t for n, t in w.items()}

    def comp16():
        with torch.autocast("cuda", dtype=torch.float16):
            return rl.sep_gru(p, h, x)
    g32, g16 = dvccorr.SepConvGRU(w, "fp32"), dvccorr.SepConvGRU(w, "fp16")
    paths = {"hip_fp32": lambda: g32(h, x), "torch_fp32": lambda: rl.sep_gru(p, h, x),
             "hip_fp16": lambda: g16(h, x), "torch_fp16": comp16}
    times = {k: [] for k in paths}
    with torch.no_grad():
        outs = {k: f().float() for k, f in paths.items()}
        ref = outs["torch_fp32"]
        err = {k: float((v - ref).abs().max() / ref.abs().max()) for k, v in outs.items()}
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
    flop = 9 * 2 * S ** 3 * 5 * (hid + inp) * hid
    res = {"shape": [1, hid + inp, S, S, S], "reps": a.reps, "warmup": a.warmup, "flop": flop,
           "device": torch.cuda.get_device_name(0), "paths": {}}
    for k, t in times.items():
        med = statistics.median(t)
        res["paths"][k] = {"median_ms": med, "min_ms": min(t), "max_ms": max(t), "tflops": flop / med / 1e9,
                           "mfma_share": flop / (med * 1e-3) / BF16_PEAK, "err_vs_torch_fp32": err[k]}
    res["hip_median_below_torch_min"] = {q: res["paths"]["hip_" + q]["median_ms"] < res["paths"]["torch_" + q]["min_ms"]
                                         for q in ("fp32", "fp16")}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
