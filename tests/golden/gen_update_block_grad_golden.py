#!/usr/bin/env python3
"""Generate the gradient fixture of the whole update block (updblk_grad_b2_597.npz, updblk_grad_b2_597_w.npz) by
importing the reference (a checkout of zachtong/RAFT-DVC).

    python tests/golden/gen_update_block_grad_golden.py --reference PATH

The reference's BasicUpdateBlock(4, 4, 96, 64, True, mode) (src/core/update.py:256-348) runs on the CPU in float32 with
the parameters of tests/update_cases.params() and the inputs of case upd_b2_597 (B = 2, volume 5 x 9 x 7: every one of
convf1's 343 taps lies inside the volume for some voxel), except that the flow is prng.uniform(FLOW_SEED, .., -2, 2)
(see below), and torch autograd differentiates one loss:

    sum(c_net * net) + sum(c_delta * delta_flow) (+ sum(c_b * log_b) with an uncertainty head),
    c_* = prng.uniform(seed, shape, -1, 1) with the seeds NET_SEED, DELTA_SEED, B_SEED

Stored in updblk_grad_b2_597.npz: seeds (NET_SEED, DELTA_SEED, B_SEED, FLOW_SEED); d_net, d_context and d_cor (the
gradient at relu(convc1(corr)), read at encoder.conv's input) in full; convf1_dw, convf1_db in full; every other bias
gradient as db.<name>.  In updblk_grad_b2_597_w.npz (a second file keeps each under 1 MB, as upd_*_enc / _head do): the
weight gradients of the other layers and of the GRU as dw8.<name>, output channels 0, 8, 16, ...  Only reference
OUTPUTS are written; no reference source is stored.

The flow seed.  A ReLU whose pre-activation is within rounding distance of zero may land on either side in another
implementation, and the gradients then differ by whole terms.  The generator ASSERTS that no pre-activation of a ReLU
that the block computes from the stored inputs (convf1, convf2, encoder.conv, flow_head.conv1, uncertainty_head.conv1)
lies within 1e-5 x max|activation| of zero (per layer).  convc1's ReLU is not among them: the tests pass cor, that
ReLU's output, and d_cor is the gradient at cor, so its mask enters no stored tensor.  Case upd_b2_597's own flow seed
(8113) violates the check, as most seeds do (about 2e5 pre-activations, each within the band with probability about 2e-5);
`--search` walks seeds upwards from 8140 and prints the first that holds, 9505.  FLOW_SEED is that seed.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "raft-dvc_amd"))

import prng  # noqa: E402
import update_cases as uc  # noqa: E402

CASE = "upd_b2_597"
NET_SEED, DELTA_SEED, B_SEED = 8151, 8152, 8153
FLOW_SEED, SEARCH_FROM = 9505, 8140
MARGIN = 1e-5
RELU_LAYERS = ("encoder.convf1", "encoder.convf2", "encoder.conv", "flow_head.conv1", "uncertainty_head.conv1")


def build_block(BasicUpdateBlock):
    B, vol, mode, _ = uc.case_meta(CASE)
    blk = BasicUpdateBlock(4, 4, 96, 64, True, mode).eval()
    p = uc.params(CASE)
    with torch.no_grad():
        for name, t in blk.named_parameters():
            t.copy_(p[name])
    return blk


def run(blk, flow_seed, backward):
    """One forward (and backward) of the reference block; returns (margins per ReLU layer, captured tensors)."""
    B, vol, mode, _ = uc.case_meta(CASE)
    c = uc.case(CASE)
    flow = torch.from_numpy(prng.uniform(flow_seed, (B, 3) + vol, -2.0, 2.0))
    pre, cap, handles = {}, {}, []
    mods = dict(blk.named_modules())
    for layer in RELU_LAYERS:
        if layer in mods:
            handles.append(mods[layer].register_forward_hook(
                lambda m, i, out, layer=layer: pre.__setitem__(layer, out.detach().clone())))   # FlowHead's ReLU is in place

    def keep_input(m, args):
        if args[0].requires_grad:
            args[0].retain_grad()
        cap["enc_in"] = args[0]
    handles.append(blk.encoder.conv.register_forward_pre_hook(keep_input))
    net = c["net0"].clone().requires_grad_(backward)
    context = c["context"].clone().requires_grad_(backward)
    with torch.set_grad_enabled(backward):
        net1, delta, log_b = blk(net, context, c["corr"], flow)
        if backward:
            loss = (torch.from_numpy(prng.uniform(NET_SEED, tuple(net1.shape), -1.0, 1.0)) * net1).sum() \
                + (torch.from_numpy(prng.uniform(DELTA_SEED, tuple(delta.shape), -1.0, 1.0)) * delta).sum()
            if log_b is not None:
                loss = loss + (torch.from_numpy(prng.uniform(B_SEED, tuple(log_b.shape), -1.0, 1.0)) * log_b).sum()
            loss.backward()
    for h in handles:
        h.remove()
    margins = {l: float(a.abs().min() / a.clamp(min=0).max()) for l, a in pre.items()}
    cap.update(net=net, context=context)
    return margins, cap


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference repository")
    ap.add_argument("--search", action="store_true", help="print the first flow seed >= SEARCH_FROM that passes the check")
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    from src.core.update import BasicUpdateBlock  # type: ignore
    blk = build_block(BasicUpdateBlock)
    if a.search:
        for seed in range(SEARCH_FROM, SEARCH_FROM + 20000):
            margins, _ = run(blk, seed, False)
            if min(margins.values()) > MARGIN:
                print("flow seed", seed, margins)
                return
        raise SystemExit("no seed found")
    margins, cap = run(blk, FLOW_SEED, True)
    print("min |pre-activation| / max activation:", margins)
    assert min(margins.values()) > MARGIN, margins
    grads = {n: t.grad for n, t in blk.named_parameters()}
    full = dict(seeds=np.array((NET_SEED, DELTA_SEED, B_SEED, FLOW_SEED)), d_net=cap["net"].grad.numpy(),
                d_context=cap["context"].grad.numpy(), d_cor=cap["enc_in"].grad[:, :96].numpy(),
                convf1_dw=grads["encoder.convf1.weight"].numpy(), convf1_db=grads["encoder.convf1.bias"].numpy())
    strided = {}
    for n, g in grads.items():
        if n.startswith("encoder.convf1.") or n.startswith("encoder.convc1."):
            continue
        if n.endswith(".bias"):
            full["db." + n[:-5]] = g.numpy()
        else:
            strided["dw8." + n[:-7]] = g[::8].numpy()
    for fname, arrays in (("updblk_grad_b2_597.npz", full), ("updblk_grad_b2_597_w.npz", strided)):
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **{k: np.ascontiguousarray(v) for k, v in arrays.items()})
        size = os.path.getsize(path)
        assert size < 1_000_000, (path, size)
        print("wrote", path, size, "bytes")


if __name__ == "__main__":
    main()
