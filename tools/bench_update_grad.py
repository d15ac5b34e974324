#!/usr/bin/env python3
"""Time the training path of the update block at (1, ., 32, 32, 32), all in one process:

  convf1    the HIP backward of dvccorr::conv7_ad (k_conv3_grad_prep + k_conv7_wgrad, one timed region, and the weight
            gradient alone) against the library's backward of the same layer (torch.autograd.grad through F.conv3d +
            ReLU for the weight and the bias; the flow is detached in the model and asks for no gradient), in fp32 and
            in fp16 (the library under torch.autocast);
  block     dvccorr.update_block_ad forward + backward (every parameter, net, context and cor) against the same block
            built from F.conv3d calls (tests/raftdvc_loop.py), in fp32 and in fp16 (the library under torch.autocast).

    python tools/bench_update_grad.py [--reps 30] [--warmup 5] [--out profiles/r11/update_grad_bench.json]

The protocol is tools/bench_conv3_grad.py's: every repetition is timed with a pair of device events and all paths
alternate inside each repetition.  The errors of convf1's dW (max-normalised, fp32 / fp16 / bf16) are against F.conv3d
in float64 on the GPU with the ReLU mask of the HIP forward's own output; the two fp32 blocks' gradients are compared
with the same block in float64 on the GPU, worst tensor of each: every block with its own ReLU masks, and the HIP
block also against float64 under the HIP forward's masks (a mask bit that differs moves a weight gradient by a whole
term, which is why the tests take the mask from the op's own output)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "update_grad_bench.json"))
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("at least 20 timed repetitions")
    import dvccorr
    from dvccorr import ops
    import prng
    import raftdvc_loop as rl
    dev = torch.device("cuda:0")
    S = a.size
    vol = (S, S, S)
    p = rl.load_params(dev)
    paths, errs = {}, {}

    def rnd(seed, c, bound=1.0):
        return torch.from_numpy(prng.uniform(seed, (1, c, *vol), -bound, bound)).to(dev)

    # ---- convf1's backward ----
    w, b = p["encoder.convf1.weight"], p["encoder.convf1.bias"]
    flow, gy = rnd(9501, 3, 2.0), rnd(9502, 64)
    for name, half in (("torch_fp32", False), ("torch_fp16", True)):
        ws, bs = (t.detach().clone().requires_grad_(True) for t in (w, b))
        with torch.autocast("cuda", dtype=torch.float16, enabled=half):
            y = F.relu(F.conv3d(flow, ws, bs, padding=3))
        paths[f"convf1/{name}"] = lambda y=y, leaves=(ws, bs): torch.autograd.grad(y, leaves, gy.to(y.dtype),
                                                                                   retain_graph=True)
    for prec in ("fp32", "fp16", "bf16"):
        dtype = ops.dtype_code(prec)
        y = torch.empty((1, 64, *vol), device=dev)
        ops.conv7_flow(flow, ops.conv7_flow_pack(w, b, dtype), y, dtype)
        g = ops.conv3_grad_prep(gy, y, True)[0]

        def wgrad(g=g, dtype=dtype):
            return ops.conv7_wgrad(flow, g, dtype)

        def backward(y=y, dtype=dtype):
            gg, db = ops.conv3_grad_prep(gy, y, True)
            return ops.conv7_wgrad(flow, gg, dtype), db
        ws = w.double().requires_grad_(True)
        rw, = torch.autograd.grad(F.conv3d(flow.double(), ws, b.double(), padding=3), (ws,), g.double())
        dw = backward()[0]
        errs[f"convf1/{prec}"] = {"dw": float((dw.double() - rw).abs().max() / rw.abs().max())}
        del ws, rw
        if prec != "bf16":
            paths[f"convf1/hip_{prec}"], paths[f"convf1/hip_{prec}_wgrad"] = backward, wgrad

    # ---- the whole block, forward + backward ----
    pg = {n: t.detach().clone().requires_grad_(True) for n, t in p.items()}
    net, ctx, cor = (t.requires_grad_(True) for t in (rnd(9511, 96), torch.relu(rnd(9512, 64)), torch.relu(rnd(9513, 96))))
    c_net, c_delta = rnd(9514, 96), rnd(9515, 3)
    leaves = [t for n, t in pg.items() if not n.startswith("encoder.convc1.")] + [net, ctx, cor]

    def hip_block(prec):
        n1, delta, _ = dvccorr.update_block_ad(net, ctx, flow, pg, cor=cor, precision=prec)
        return torch.autograd.grad((c_net * n1).sum() + (c_delta * delta).sum(), leaves)

    def torch_block(half):
        with torch.autocast("cuda", dtype=torch.float16, enabled=half):
            n1, delta = rl.update_block(pg, net, ctx, flow, cor=cor)
        return torch.autograd.grad((c_net * n1.float()).sum() + (c_delta * delta.float()).sum(), leaves)
    for prec, half in (("fp32", False), ("fp16", True)):
        paths[f"block/hip_{prec}"] = lambda prec=prec: hip_block(prec)
        paths[f"block/torch_{prec}"] = lambda half=half: torch_block(half)
    # both fp32 blocks against the same block in float64 on the GPU: the worst gradient tensor of each.  A ReLU whose
    # pre-activation is within the forward's error of zero may land on either side, and a weight gradient then differs by
    # a whole term; so the HIP block is also compared with the float64 block under the HIP forward's own ReLU masks.
    names = [n for n in pg if not n.startswith("encoder.convc1.")] + ["net", "context", "cor"]
    p64 = {n: t.detach().double().requires_grad_(True) for n, t in pg.items()}
    i64 = [t.detach().double().requires_grad_(True) for t in (net, ctx, cor)]
    f64 = flow.double()

    def block64(masks):
        act = (lambda x, k: x * masks[k]) if masks else (lambda x, k: F.relu(x))
        flo = act(rl._conv(p64, "encoder.convf1", f64, 3), "flo1")
        flo = act(rl._conv(p64, "encoder.convf2", flo, 1), "flo2")
        mot = act(rl._conv(p64, "encoder.conv", torch.cat([i64[2], flo], dim=1), 1), "mot")
        n64 = rl.sep_gru(p64, i64[0], torch.cat([i64[1], mot, f64], dim=1))
        d64 = rl._conv(p64, "flow_head.conv2", act(rl._conv(p64, "flow_head.conv1", n64, 1), "hid"), 1)
        grads = torch.autograd.grad((c_net.double() * n64).sum() + (c_delta.double() * d64).sum(),
                                    [p64[n] for n in names[:-3]] + i64)
        return grads

    def worst_error(got, ref):
        e = {n: float((x.double() - r).abs().max() / r.abs().max()) for n, x, r in zip(names, got, ref)}
        worst = max(e, key=e.get)
        return {"max": e[worst], "worst": worst}
    with torch.no_grad():
        wb = lambda l: (pg[l + ".weight"], pg[l + ".bias"])   # noqa: E731
        h1 = dvccorr.conv7x7x7_flow_ad(flow, *wb("encoder.convf1"), precision="fp32")
        h2 = dvccorr.conv3x3x3_ad(h1, *wb("encoder.convf2"), relu=True, precision="fp32")
        hm = dvccorr.conv3x3x3_ad(cor, *wb("encoder.conv"), relu=True, precision="fp32", x2=h2)
        hn = dvccorr.sep_conv_gru_ad(net, torch.cat([ctx, hm, flow], dim=1),
                                     {n[4:]: t for n, t in pg.items() if n.startswith("gru.")}, precision="fp32")
        hh = dvccorr.conv3x3x3_ad(hn, *wb("flow_head.conv1"), relu=True, precision="fp32")
        masks = {k: (v > 0).double() for k, v in (("flo1", h1), ("flo2", h2), ("mot", hm), ("hid", hh))}
    ref = block64(None)
    got = hip_block("fp32")
    errs["block/hip_fp32"] = worst_error(got, ref)
    errs["block/torch_fp32"] = worst_error(torch_block(False), ref)
    errs["block/hip_fp32_under_its_own_masks"] = worst_error(got, block64(masks))
    del ref, got, masks, p64, i64, h1, h2, hm, hn, hh

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
           "convf1_wgrad_flop": 2 * S ** 3 * 343 * 3 * 64, "slabs": list(ops.conv7_wgrad_slabs(1, *vol)),
           "errors": errs, "paths": {}}
    for k, t in times.items():
        res["paths"][k] = {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)}
    res["summary"] = {}
    for what in ("convf1", "block"):
        for prec in ("fp32", "fp16"):
            hip, lib = res["paths"][f"{what}/hip_{prec}"], res["paths"][f"{what}/torch_{prec}"]
            res["summary"][f"{what}/{prec}"] = {"hip_median_ms": hip["median_ms"], "torch_median_ms": lib["median_ms"],
                                                "torch_min_ms": lib["min_ms"],
                                                "hip_median_below_torch_min": hip["median_ms"] < lib["min_ms"]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
