#!/usr/bin/env python3
"""Time forward + backward of dvccorr.encoder_ad([v0, v1]) and dvccorr.context_encoder_ad(v0) for the 1/8 encoder
against the same nn.Module.

    python tools/bench_encoder_grad.py [--sizes 64 128] [--reps 10] [--warmup 3]
                                       [--out profiles/r13/encoder_grad_bench.json]

Per size (a cubic input volume) and precision (fp32, fp16): one training step of the encoder alone (forward, a fixed
G-weighted sum as the loss, backward to every convolution weight and bias) on the HIP path, and the same step of the
restated nn.Module of tests/raftdvc_encoder.py in float32 and under torch.autocast(float16), in one process,
alternating.  Times are medians of `reps` calls after `warmup` calls, each bracketed by device events and ended by a
synchronise; the spread (min, max) is kept.  Per-kernel sums come from torch.profiler over three further calls, taken
after the end-to-end numbers.  The clocks are whatever the device settles at under this load: compare numbers of one
run only.  A size that does not fit memory is recorded as skipped, with the error.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raft-dvc_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_encoder import _kernels, _time  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "encoder_grad_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_encoder_grad: no GPU (times are taken on the MI355X only)")
    import dvccorr
    import raftdvc_encoder as renc
    dev = torch.device("cuda:0")
    fnet = renc.Encoder("1/8", output_dim=128).eval()
    renc.set_params(fnet, 100)
    cnet = renc.Encoder("1/8", output_dim=160).eval()
    for m in cnet.modules():   # norm_fn = 'none'
        for n in ("norm1", "norm2", "norm3", "norm4"):
            if isinstance(getattr(m, n, None), torch.nn.InstanceNorm3d):
                setattr(m, n, torch.nn.Identity())
        if getattr(m, "downsample", None) is not None and not isinstance(m, torch.nn.Sequential):
            m.downsample[1] = torch.nn.Identity()
    renc.set_params(cnet, 200)
    fnet, cnet = fnet.to(dev), cnet.to(dev)
    fsd = fnet.state_dict(keep_vars=True)
    csd = {"encoder." + k: v for k, v in cnet.state_dict(keep_vars=True).items()}
    params = list(fnet.parameters()) + list(cnet.parameters())
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "lib": dvccorr.LIB_PATH.split("/")[-1],
           "encoder": "1/8", "what": "forward + backward, ms", "cases": []}
    g = torch.Generator(device="cpu").manual_seed(1)
    for S in a.sizes:
        rec = {"size": S}
        try:
            v0 = torch.rand((1, 1, S, S, S), generator=g).to(dev)
            v1 = torch.rand((1, 1, S, S, S), generator=g).to(dev)
            o = -(-S // 8)
            G = torch.rand((1, 160, o, o, o), generator=g).to(dev) / (160 * o ** 3)

            def step(outs):
                for p in params:
                    p.grad = None
                sum((y * G[:, :y.shape[1]]).sum() for y in outs).backward()

            for prec, ac in (("fp32", None), ("fp16", torch.float16)):
                def lib_f():
                    with torch.autocast("cuda", dtype=ac or torch.float16, enabled=ac is not None):
                        y = fnet(torch.cat([v0, v1]))
                    step(torch.split(y, [1, 1]))

                def lib_c():
                    with torch.autocast("cuda", dtype=ac or torch.float16, enabled=ac is not None):
                        y = cnet(v0)
                        outs = (torch.tanh(y[:, :96]), torch.relu(y[:, 96:]))
                    step(outs)

                def hip_f():
                    step(dvccorr.encoder_ad([v0, v1], fsd, "1/8", "instance", prec))

                def hip_c():
                    step(dvccorr.context_encoder_ad(v0, csd, "1/8", "none", 96, 64, prec))

                r = {}
                for name, fn in (("hip_fnet", hip_f), ("library_fnet", lib_f), ("hip_cnet", hip_c), ("library_cnet", lib_c)):
                    r[name] = _time(fn, a.reps, a.warmup)
                r["hip_fnet_kernels_ms"] = _kernels(hip_f)
                r["hip_cnet_kernels_ms"] = _kernels(hip_c)
                r["library_fnet_kernels_ms"] = _kernels(lib_f)
                rec[prec] = r
                print(S, prec, {k: round(v["median_ms"], 3) for k, v in r.items() if "median_ms" in v}, flush=True)
                torch.cuda.empty_cache()
        except (RuntimeError, torch.cuda.OutOfMemoryError) as e:   # memory allowing
            rec["skipped"] = str(e).splitlines()[0][:200]
            print(S, "skipped:", rec["skipped"], flush=True)
            torch.cuda.empty_cache()
        res["cases"].append(rec)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"out": a.out, "cases": len(res["cases"])}))


if __name__ == "__main__":
    main()
