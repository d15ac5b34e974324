#!/usr/bin/env python3
"""Time dvccorr.Encoder([v0, v1]) and dvccorr.ContextEncoder(v0) for the 1/8 encoder against the same nn.Module.

    python tools/bench_encoder.py [--sizes 64 128 256] [--reps 10] [--warmup 3] [--out profiles/r12/encoder_bench.json]

Per size (a cubic input volume) and precision (fp32, fp16): the HIP objects, and the library composition (the
restated nn.Module of tests/raftdvc_encoder.py in eval mode) in float32 and under torch.autocast(float16), in this
process and session.  Times are medians of `reps` calls after `warmup` calls, each bracketed by device events and
ended by a synchronise; the spread (min, max) is kept.  Per-kernel times come from torch.profiler over three further
calls (kernel names k_enc_*), taken after the end-to-end numbers so that tracing does not slow them.  The clocks are
whatever the device settles at under this load: compare numbers of one run only.  A size that does not fit memory is
recorded as skipped, with the error.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raft-dvc_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _time(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": reps}


def _kernels(fn, calls=3):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.key_averages():
        t = getattr(e, "device_time_total", None)
        if t is None:
            t = getattr(e, "cuda_time_total", 0.0)
        if t > 0:
            name = e.key.split("(")[0][:80]
            out[name] = out.get(name, 0.0) + t / 1000.0 / calls
    return dict(sorted(out.items(), key=lambda kv: -kv[1])[:12])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "encoder_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_encoder: no GPU (times are taken on the MI355X only)")
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
    fsd = {k: v.detach() for k, v in fnet.state_dict().items()}
    csd = {"encoder." + k: v.detach() for k, v in cnet.state_dict().items()}
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "lib": dvccorr.LIB_PATH.split("/")[-1],
           "encoder": "1/8", "cases": []}
    g = torch.Generator(device="cpu").manual_seed(1)
    for S in a.sizes:
        rec = {"size": S}
        try:
            v0 = torch.rand((1, 1, S, S, S), generator=g).to(dev)
            v1 = torch.rand((1, 1, S, S, S), generator=g).to(dev)
            with torch.no_grad():
                for prec, ac in (("fp32", None), ("fp16", torch.float16)):
                    enc = dvccorr.Encoder(fsd, "1/8", "instance", precision=prec)
                    cenc = dvccorr.ContextEncoder(csd, "1/8", "none", precision=prec)

                    def lib_f():
                        with torch.autocast("cuda", dtype=ac or torch.float16, enabled=ac is not None):
                            return fnet(torch.cat([v0, v1]))

                    def lib_c():
                        with torch.autocast("cuda", dtype=ac or torch.float16, enabled=ac is not None):
                            y = cnet(v0)
                            return torch.tanh(y[:, :96]), torch.relu(y[:, 96:])
                    r = {"hip_fnet": _time(lambda: enc([v0, v1]), a.reps, a.warmup),
                         "hip_cnet": _time(lambda: cenc(v0), a.reps, a.warmup),
                         "library_fnet": _time(lib_f, a.reps, a.warmup),
                         "library_cnet": _time(lib_c, a.reps, a.warmup)}
                    r["hip_fnet_kernels_ms"] = _kernels(lambda: enc([v0, v1]))
                    r["hip_cnet_kernels_ms"] = _kernels(lambda: cenc(v0))
                    rec[prec] = r
                    print(S, prec, {k: round(v["median_ms"], 3) for k, v in r.items() if "median_ms" in v}, flush=True)
                    del enc, cenc
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
