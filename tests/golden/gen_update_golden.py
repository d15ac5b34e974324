#!/usr/bin/env python3
"""Generate the BasicUpdateBlock fixtures (upd_*_enc.npz, upd_*_head.npz, update_meta.json) by importing the
reference (a checkout of zachtong/RAFT-DVC).

    python tests/golden/gen_update_golden.py --reference PATH

The reference's BasicUpdateBlock(4, 4, 96, 64, True, mode) (src/core/update.py:256-348) runs on the CPU in float32.
Its parameters are set from the portable PRNG (tests/prng.py) with epe_meta.json's seeds and bounds (the closed-loop
fixture's update block); the uncertainty head's four parameters, which that fixture does not have, get new seeds and
the same rule, uniform(-b, b) with b = 1/sqrt(fan_in), written to update_meta.json.  Per case net = prng.uniform(-1, 1),
context = relu(prng.normal), flow = prng.uniform(-2, 2), corr = 0.5 prng.normal; tests regenerate all four and the
parameters from the seeds.

Stored per case, split over two files to keep each under 1 MB -- NAME_enc.npz: shape, seeds, cor (relu(convc1)),
flo1 (relu(convf1)), flo2 (relu(convf2)), motion_features (the encoder's output, cat[relu(conv), flow]);
NAME_head.npz: net (the GRU's output), hid (relu(flow_head.conv1)), delta_flow and, with an uncertainty head,
unc_hid (relu(uncertainty_head.conv1)) and log_b.  Only reference OUTPUTS are written; no reference source is stored.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))

import prng  # noqa: E402

UNC_SEED_BASE = 7180
# name, B, (H, W, D), uncertainty mode, seeds of net, context, flow, corr
CASES = (("upd_888", 1, (8, 8, 8), "none", (8101, 8102, 8103, 8104)),        # baseline cube
         ("upd_b2_597", 2, (5, 9, 7), "none", (8111, 8112, 8113, 8114)),     # odd, non-cubic, batch stride
         ("upd_215", 1, (2, 1, 5), "mol", (8121, 8122, 8123, 8124)))         # axes shorter than the taps, 4-channel head


def case_inputs(B, vol, seeds, corr_planes=2916):
    """(net, context, flow, corr) float32 arrays of one case; tests/update_cases.py restates this."""
    sn, sc, sf, sr = seeds
    net = prng.uniform(sn, (B, 96) + tuple(vol), -1.0, 1.0)
    context = np.maximum(prng.normal(sc, (B, 64) + tuple(vol)), 0.0).astype(np.float32)
    flow = prng.uniform(sf, (B, 3) + tuple(vol), -2.0, 2.0)
    corr = (0.5 * prng.normal(sr, (B, corr_planes) + tuple(vol))).astype(np.float32)
    return net, context, flow, corr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference repository")
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    from src.core.update import BasicUpdateBlock  # type: ignore
    with open(os.path.join(HERE, "epe_meta.json")) as f:
        epe = {name: (shape, seed, b) for name, shape, seed, b in json.load(f)["params"]}
    unc_meta = {}
    for name, B, vol, mode, seeds in CASES:
        blk = BasicUpdateBlock(4, 4, 96, 64, True, mode).eval()
        named = dict(blk.named_parameters())
        i = 0
        with torch.no_grad():
            for pname, p in named.items():
                if pname in epe:
                    shape, seed, bound = epe[pname]
                    assert list(p.shape) == list(shape), (pname, p.shape, shape)
                else:
                    w = named[pname.rsplit(".", 1)[0] + ".weight"]
                    bound = 1.0 / float(np.sqrt(w.shape[1] * int(np.prod(w.shape[2:]))))
                    seed = UNC_SEED_BASE + i
                    i += 1
                    unc_meta[mode] = unc_meta.get(mode, []) + [(pname, list(p.shape), seed, bound)]
                p.copy_(torch.from_numpy(prng.uniform(seed, tuple(p.shape), -bound, bound)))
        cap = {}

        def keep(key, relu):
            def hook(m, inp, out):
                cap[key] = (torch.relu(out) if relu else out).detach().numpy().copy()
            return hook
        blk.encoder.convc1.register_forward_hook(keep("cor", True))
        blk.encoder.convf1.register_forward_hook(keep("flo1", True))
        blk.encoder.convf2.register_forward_hook(keep("flo2", True))
        blk.encoder.register_forward_hook(keep("motion_features", False))
        blk.flow_head.conv1.register_forward_hook(keep("hid", True))
        if blk.uncertainty_head is not None:
            blk.uncertainty_head.conv1.register_forward_hook(keep("unc_hid", True))
        net, context, flow, corr = (torch.from_numpy(v) for v in case_inputs(B, vol, seeds))
        with torch.no_grad():
            net1, delta, log_b = blk(net, context, corr, flow)
        enc = dict(shape=np.array((B,) + vol), seeds=np.array(seeds), cor=cap["cor"], flo1=cap["flo1"],
                   flo2=cap["flo2"], motion_features=cap["motion_features"])
        head = dict(net=net1.numpy(), hid=cap["hid"], delta_flow=delta.numpy())
        if log_b is not None:
            head.update(unc_hid=cap["unc_hid"], log_b=log_b.numpy())
        for suffix, arrays in (("enc", enc), ("head", head)):
            path = os.path.join(HERE, f"{name}_{suffix}.npz")
            np.savez_compressed(path, **arrays)
            size = os.path.getsize(path)
            assert size < 1_000_000, (path, size)
            print("wrote", path, size, "bytes")
    with open(os.path.join(HERE, "update_meta.json"), "w") as f:
        json.dump({"torch": torch.__version__,
                   "config": "BasicUpdateBlock(4, 4, 96, 64, True, mode), float32 on the CPU; parameters of "
                             "epe_meta.json, the uncertainty head's below (uniform(-b, b) from tests/prng.py)",
                   "uncertainty_params": unc_meta,
                   "cases": [[c[0], c[1], list(c[2]), c[3], list(c[4])] for c in CASES]}, f, indent=1)


if __name__ == "__main__":
    main()
