#!/usr/bin/env python3
"""Golden outputs of the reference ContextEncoder for tests/test_gpu_encoder.py -- survey container only.

    python tests/golden/gen_context_encoder_golden.py [--reference /root/reference]

ContextEncoder (zachtong/RAFT-DVC src/core/extractor.py:259-301: a BasicEncoder with norm_fn = 'none', then tanh on
the first hidden_dim channels and ReLU on the other context_dim), its parameters set from the portable PRNG
(tests/raftdvc_encoder.set_params, the seeds and order of the restatement), run in eval mode on a seeded input volume.
Only the two outputs and the seeds are stored (context_encoder_1_8.npz).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import prng  # noqa: E402
import raftdvc_encoder as renc  # noqa: E402

HIDDEN, CONTEXT, SHAPE, SEED0, IN_SEED = 96, 64, (1, 1, 32, 24, 16), 8800, 8801


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    from src.core import extractor  # type: ignore
    ref = extractor.ContextEncoder(input_dim=1, hidden_dim=HIDDEN, context_dim=CONTEXT, norm_fn="none").eval()
    mine = renc.Encoder("1/8", output_dim=HIDDEN + CONTEXT)
    assert [n for n, _ in ref.named_parameters()] == ["encoder." + n for n, _ in mine.named_parameters()]
    renc.set_params(ref, SEED0)
    x = torch.from_numpy(prng.uniform(IN_SEED, SHAPE))
    with torch.no_grad():
        net, context = ref(x)
    print("net", tuple(net.shape), "context", tuple(context.shape))
    np.savez_compressed(os.path.join(HERE, "context_encoder_1_8.npz"), net=net.numpy(), context=context.numpy(),
                        seed0=np.array([SEED0]), in_seed=np.array([IN_SEED]), in_shape=np.array(SHAPE),
                        hidden_dim=np.array([HIDDEN]), context_dim=np.array([CONTEXT]))


if __name__ == "__main__":
    main()
