#!/usr/bin/env python3
"""Generate the gradient fixture of the update block's 3 x 3 x 3 layers (updgrad_215.npz) by importing the reference
(a checkout of zachtong/RAFT-DVC).

    python tests/golden/gen_update_grad_golden.py --reference PATH

The reference's FlowHead(96, 128) and the `conv` layer of MotionEncoder(4, 4, 80) (src/core/update.py:17-38,
205-253) run on the CPU in float32 with the parameters of tests/update_cases.params() and the stored activations of
case upd_215 (volume 2 x 1 x 5) as inputs, and torch autograd differentiates two losses:

    head     sum(c_head * flow_head(net)),                    c_head = prng.uniform(HEAD_SEED, (1, 3, 2, 1, 5), -1, 1)
    encoder  sum(c_enc * relu(encoder.conv(cat[cor, flo2]))), c_enc  = prng.uniform(ENC_SEED, (1, 80, 2, 1, 5), -1, 1)

Stored: d_net; conv2_dw, conv2_db; conv1_db and conv1_dw8 (output channels 0, 8, 16, ..); d_cor, d_flo2; enc_db and
enc_dw8 (output channels 0, 8, ..); the two seeds.  Only reference OUTPUTS are written; no reference source is stored.
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

CASE = "upd_215"
HEAD_SEED, ENC_SEED = 8131, 8132


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference repository")
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    from src.core.update import FlowHead, MotionEncoder  # type: ignore
    p, c = uc.params(CASE), uc.case(CASE)
    head, enc = FlowHead(96, 128), MotionEncoder(4, 4, 80)
    with torch.no_grad():
        for mod, prefix in ((head.conv1, "flow_head.conv1"), (head.conv2, "flow_head.conv2"),
                            (enc.conv, "encoder.conv")):
            mod.weight.copy_(p[prefix + ".weight"])
            mod.bias.copy_(p[prefix + ".bias"])
    net = c["net"].clone().requires_grad_(True)
    c_head = torch.from_numpy(prng.uniform(HEAD_SEED, tuple(c["delta_flow"].shape), -1.0, 1.0))
    (c_head * head(net)).sum().backward()
    cor, flo2 = c["cor"].clone().requires_grad_(True), c["flo2"].clone().requires_grad_(True)
    c_enc = torch.from_numpy(prng.uniform(ENC_SEED, tuple(c["motion"].shape), -1.0, 1.0))
    (c_enc * torch.relu(enc.conv(torch.cat([cor, flo2], dim=1)))).sum().backward()
    out = dict(seeds=np.array((HEAD_SEED, ENC_SEED)), d_net=net.grad.numpy(),
               conv2_dw=head.conv2.weight.grad.numpy(), conv2_db=head.conv2.bias.grad.numpy(),
               conv1_dw8=head.conv1.weight.grad[::8].numpy(), conv1_db=head.conv1.bias.grad.numpy(),
               d_cor=cor.grad.numpy(), d_flo2=flo2.grad.numpy(),
               enc_dw8=enc.conv.weight.grad[::8].numpy(), enc_db=enc.conv.bias.grad.numpy())
    path = os.path.join(HERE, "updgrad_215.npz")
    np.savez_compressed(path, **{k: np.ascontiguousarray(v) for k, v in out.items()})
    size = os.path.getsize(path)
    assert size < 1_000_000, (path, size)
    print("wrote", path, size, "bytes")


if __name__ == "__main__":
    main()
