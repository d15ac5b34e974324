#!/usr/bin/env python3
"""Generate the SepConvGRU3D fixtures (gru_*.npz, gru_meta.json) -- survey container only, by importing the
reference.

    python tests/golden/gen_gru_golden.py [--reference /root/reference]

The reference's SepConvGRU3D (src/core/update.py:139-199; hidden 96, input 147 as BasicUpdateBlock builds it,
update.py:283-297) runs on the CPU in float32.  Its eighteen parameters are set from the portable PRNG
(tests/prng.py): uniform(-b, b), b = 1/sqrt(fan_in) of the owning Conv3d, one seed per parameter in
named_parameters() order (written to gru_meta.json, shared by all cases).  Per case h = prng.uniform(-1, 1) and
x = prng.normal; tests regenerate both and the parameters from the seeds.

Stored per case: the shape, the seeds and the reference's hidden state after each of the three passes (the inputs of
convz_w / convz_d are cat[h, x] after the h / w pass; the module's output is h after the d pass).  Only reference
OUTPUTS are written; no reference source is stored.
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

HIDDEN, INPUT = 96, 147
SEED_BASE = 7300
# name, B, (H, W, D), seed of h, seed of x
CASES = (("gru_888", 1, (8, 8, 8), 7401, 7402),         # baseline cube
         ("gru_b2_597", 2, (5, 9, 7), 7403, 7404),      # odd, non-cubic, batch stride
         ("gru_215", 1, (2, 1, 5), 7405, 7406))         # axes shorter than the 5 taps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    from src.core.update import SepConvGRU3D  # type: ignore
    gru = SepConvGRU3D(HIDDEN, INPUT).eval()
    meta = []
    with torch.no_grad():
        for i, (name, p) in enumerate(gru.named_parameters()):
            w = dict(gru.named_parameters())[name.rsplit(".", 1)[0] + ".weight"]
            bound = 1.0 / float(np.sqrt(w.shape[1] * int(np.prod(w.shape[2:]))))
            meta.append((name, list(p.shape), SEED_BASE + i, bound))
            p.copy_(torch.from_numpy(prng.uniform(SEED_BASE + i, tuple(p.shape), -bound, bound)))
    cap = {}
    gru.convz_w.register_forward_hook(lambda m, inp, out: cap.__setitem__("h", inp[0][:, :HIDDEN].numpy().copy()))
    gru.convz_d.register_forward_hook(lambda m, inp, out: cap.__setitem__("w", inp[0][:, :HIDDEN].numpy().copy()))
    for name, B, vol, sh, sx in CASES:
        h = torch.from_numpy(prng.uniform(sh, (B, HIDDEN) + vol, -1.0, 1.0))
        x = torch.from_numpy(prng.normal(sx, (B, INPUT) + vol))
        with torch.no_grad():
            out = gru(h, x).numpy()
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, shape=np.array((B, HIDDEN, INPUT) + vol), seeds=np.array([sh, sx]),
                            h_after_h=cap["h"], h_after_w=cap["w"], h_after_d=out)
        print("wrote", path, os.path.getsize(path), "bytes; |h'| max", float(np.abs(out).max()))
    with open(os.path.join(HERE, "gru_meta.json"), "w") as f:
        json.dump({"torch": torch.__version__, "config": f"SepConvGRU3D({HIDDEN}, {INPUT}), float32 on the CPU; "
                   "parameters uniform(-b, b) from tests/prng.py", "params": meta,
                   "cases": [c[0] for c in CASES]}, f, indent=1)


if __name__ == "__main__":
    main()
