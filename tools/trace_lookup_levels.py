#!/usr/bin/env python3
"""Per-unit timeline of the default tile lookup at config #3 (diagnostics library, lookup_tile.h ABL & 8 stamps), grouped
by blockIdx.y: how long the workgroups of each (tile, level) unit live and how much of that passes before their first
output row starts (stamp 5).  With the coarse path on (tuning lookup_coarse 1) unit 0 is the merged coarse unit
(levels 2 + 3; stamps 1-14 are those of its first level) and units 1, 2 are levels 0, 1; with it off unit y is level y.

    DVCCORR_LIB=.../libdvccorr_diag.so python tools/trace_lookup_levels.py [--tune lookup_coarse=0]
Prints one JSON object: per unit the median / 90 % life (us), start -> row 0 (us) and dispatch start (us)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raft-dvc_amd"))
os.environ.setdefault("DVCCORR_LIB", os.path.join(ROOT, "raft-dvc_amd", "dvccorr", "libdvccorr_diag.so"))
from dvccorr import _lib, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tune", default="")
a = ap.parse_args()
for item in filter(None, a.tune.split(",")):
    k, v = item.split("=")
    _lib.set_tuning(k, int(v))
dev = torch.device("cuda:0")
S, C, L, R = 32, 128, 4, 4
g = torch.Generator(device="cpu").manual_seed(5)
f1 = torch.randn(1, C, S, S, S, generator=g).to(dev)
f2 = torch.randn(1, C, S, S, S, generator=g).to(dev)
base = torch.stack(torch.meshgrid(*[torch.arange(S, dtype=torch.float32)] * 3, indexing="ij"))[None]
coords = (base + (torch.rand(1, 3, S, S, S, generator=g) * 4 - 2)).to(dev)
dt = ops.dtype_code("bf16")
lay = ops.layout(S, S, S, L, C)
brick = ops.DVC_BRICKED if ops.bricked_levels(lay) else 0
q = ops.pack_queries(f1.reshape(1, C, -1), dt)
t = ops.pack_targets(f2, L, dt | brick)
corr = ops.build(q, t, C, S, S, S, L, dt, dt)
cf = coords.reshape(1, 3, -1)
for _ in range(3):
    ops.lookup(corr, cf, S, S, S, L, R, False, dt | brick)
tiles = S * S * S // 64
nwg = tiles * L
buf = torch.zeros(nwg * 16, dtype=torch.int64, device=dev)
p = buf.data_ptr()
_lib.set_tuning("lookup_trace_lo", int(p & 0xffffffff) - (1 << 32 if p & 0x80000000 else 0))
_lib.set_tuning("lookup_trace_hi", int(p >> 32))
ops.lookup(corr, cf, S, S, S, L, R, False, dt | brick)
torch.cuda.synchronize()
_lib.set_tuning("lookup_trace_lo", 0)
_lib.set_tuning("lookup_trace_hi", 0)
st = buf.view(nwg, 16).cpu().numpy().astype(np.float64)
t0 = st[st[:, 0] > 0, 0].min()
res = {"lib": os.path.basename(_lib.LIB_PATH), "tune": a.tune, "kernel_us": float((st[:, 15].max() - t0) / 100.0),
       "units": {}}
for y in range(L):
    u = st[y * tiles:(y + 1) * tiles]
    u = u[u[:, 0] > 0]
    if not len(u):
        continue
    life, pre, start = (u[:, 15] - u[:, 0]) / 100.0, (u[:, 5] - u[:, 0]) / 100.0, (u[:, 0] - t0) / 100.0
    med = lambda x: [round(float(v), 2) for v in np.percentile(x, [50, 90])]
    res["units"][str(y)] = {"workgroups": int(len(u)), "life_us_q50_90": med(life), "start_to_row0_us_q50_90": med(pre),
                            "dispatched_at_us_q50_90": med(start)}
print(json.dumps(res))
