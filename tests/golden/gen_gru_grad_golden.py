#!/usr/bin/env python3
"""Generate the gradient fixture of the update block's GRU (grugrad_215.npz) by importing the reference (a checkout
of zachtong/RAFT-DVC).

    python tests/golden/gen_gru_grad_golden.py --reference PATH

The reference's SepConvGRU3D(96, 147) (src/core/update.py:139-199) runs on the CPU in float32 with the parameters of
tests/gru_cases.params() and the inputs of case gru_215 (volume 2 x 1 x 5), and torch autograd differentiates

    sum(c * gru(h, x)),    c = prng.uniform(SEED, (1, 96, 2, 1, 5), -1, 1)

Stored: d_h, d_x; every bias gradient ("<name>.bias"); output channels 0, 8, 16, .. of every weight gradient
("<name>.weight8"); the seed.  Only reference OUTPUTS are written; no reference source is stored.
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

import gru_cases  # noqa: E402
import prng  # noqa: E402

CASE = "gru_215"
SEED = 8141


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference repository")
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    from src.core.update import SepConvGRU3D  # type: ignore
    p = gru_cases.params()
    h, x, _ = gru_cases.inputs(CASE)
    gru = SepConvGRU3D(96, 147)
    gru.load_state_dict(p)
    h, x = h.clone().requires_grad_(True), x.clone().requires_grad_(True)
    c = torch.from_numpy(prng.uniform(SEED, tuple(h.shape), -1.0, 1.0))
    (c * gru(h, x)).sum().backward()
    out = dict(seed=np.array(SEED), d_h=h.grad.numpy(), d_x=x.grad.numpy())
    for n, t in gru.named_parameters():
        out[n if n.endswith(".bias") else n + "8"] = (t.grad if n.endswith(".bias") else t.grad[::8]).numpy()
    path = os.path.join(HERE, "grugrad_215.npz")
    np.savez_compressed(path, **{k: np.ascontiguousarray(v) for k, v in out.items()})
    size = os.path.getsize(path)
    assert size < 1_000_000, (path, size)
    print("wrote", path, size, "bytes")


if __name__ == "__main__":
    main()
