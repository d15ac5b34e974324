"""GPU: the bytes k_gru_pack, k_conv3_pack and k_conv7_pack write (csrc/gru.hip, csrc/conv3.hip), rebuilt in plain
torch on the CPU from the layout comments above those kernels and compared bitwise.

The fixture tests pass under any change made alike to a pack kernel and to the kernel that reads its buffer; this
test pins the layout itself, so a packed buffer kept across a reload of the library stays valid.

A packed buffer is fragments, then float32 biases.  A fragment is NP pieces of [64 lanes][8] 16-bit values (1 KB):
bf16 / fp16 one piece of the rounded weights; fp32 a bf16 hi piece, then the bf16 lo piece of v - hi.  Lane l,
value j of a fragment is the weight of output channel 16 tile + (l & 15) and K index 8 (l >> 4) + j of the fragment's
32-wide K chunk; weights past the real channel counts are zeros.

Tolerance zero: hi is the round-to-nearest-even bf16 / fp16 of the fp32 weight, as Tensor.to(torch.bfloat16) and
.half() are; v - float(hi) is exact in fp32 and lo its bf16; biases are copied.  The weights are uniform in (-1, 1)
(multiples of 2^-23), so no denormals."""
from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
PRECISIONS = ["fp32", "fp16", "bf16"]


def _uniform(seed, shape):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=torch.float32) * 2.0 - 1.0


def _packed_bytes(frags, biases, precision):
    """frags (n, 64, 8) float32, fragment-major -> the expected buffer as uint8."""
    if precision == "fp16":
        pieces = frags.half().view(torch.int16).unsqueeze(1)
    else:
        hi = frags.to(torch.bfloat16)
        pieces = hi.view(torch.int16).unsqueeze(1)
        if precision == "fp32":
            lo = (frags - hi.float()).to(torch.bfloat16)
            pieces = torch.cat([pieces, lo.view(torch.int16).unsqueeze(1)], dim=1)
    return torch.cat([pieces.contiguous().view(torch.uint8).flatten(),
                      biases.contiguous().view(torch.uint8).flatten()])


def _frags(wp, ntile, nchunk):
    """wp (16 ntile, 32 nchunk, taps), zero-padded -> fragments [chunk][tap][tile] of [lane = 16 q + m][j]."""
    taps = wp.shape[2]
    v = wp.reshape(ntile, 16, nchunk, 4, 8, taps)         # tile, m, chunk, q, j, tap
    return v.permute(2, 5, 0, 3, 1, 4).reshape(nchunk * taps * ntile, 64, 8)


def _same(got, want):
    got = got.detach().cpu().contiguous().view(torch.uint8).flatten()
    assert got.numel() == want.numel(), (got.numel(), want.numel())
    bad = (got != want).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} bytes differ, first at byte {int(bad[0])}"


# (cin, cout) -> packed tiles: the 16-channel tiles of cout, rounded up to what the kernel instance computes
# (1, 2, 4 = one FULL, 5 = FULL + SHARED, 8 = two FULL)
CONV3_CASES = {(40, 21): 2, (33, 80): 5, (32, 48): 4}


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("cin,cout", list(CONV3_CASES))
def test_conv3_pack(cin, cout, precision):
    from dvccorr import ops
    nt, nch = CONV3_CASES[(cin, cout)], (cin + 31) // 32
    w, b = _uniform(100 + cin, (cout, cin, 3, 3, 3)), _uniform(200 + cout, (cout,))
    wp = torch.zeros(16 * nt, 32 * nch, 27)
    wp[:cout, :cin] = w.reshape(cout, cin, 27)             # tap = (kh 3 + kw) 3 + kd
    bp = torch.zeros(16 * nt)
    bp[:cout] = b
    got = ops.conv3_pack(w.to(DEV), b.to(DEV), ops.dtype_code(precision))
    _same(got, _packed_bytes(_frags(wp, nt, nch), bp, precision))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_conv7_flow_pack(precision):
    from dvccorr import ops
    w, b = _uniform(301, (64, 3, 7, 7, 7)), _uniform(302, (64,))
    wp = torch.zeros(64, 4, 7, 7, 8)                       # o, ci (the fourth is zeros), kh, kw, kd (the eighth is zero)
    wp[:, :3, :, :, :7] = w
    v = wp.reshape(4, 16, 4, 7, 7, 8)                      # tile, m, ci, kh, kw, j
    frags = v.permute(3, 4, 0, 2, 1, 5).reshape(49 * 4, 64, 8)   # [kh 7 + kw][tile] of [lane = 16 ci + m][j = kd]
    got = ops.conv7_flow_pack(w.to(DEV), b.to(DEV), ops.dtype_code(precision))
    _same(got, _packed_bytes(frags, b, precision))


GRU_SHAPE = {"h": (5, 1, 1), "w": (1, 5, 1), "d": (1, 1, 5)}


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("cx", [19, 147])
def test_gru_pack(cx, precision):
    from dvccorr import ops
    hid, cin = 96, 96 + cx
    weights, seed = {}, 400 + cx
    for ax, k in GRU_SHAPE.items():
        for g in "zrq":
            seed += 1
            weights[f"conv{g}_{ax}.weight"] = _uniform(seed, (hid, cin) + k)
            weights[f"conv{g}_{ax}.bias"] = _uniform(seed + 50, (hid,))
    got = ops.gru_pack({n: t.to(DEV) for n, t in weights.items()}, ops.dtype_code(precision))
    assert got.shape[0] == 3
    for a, ax in ((0, "h"), (2, "d")):
        wz, wr, wq = (weights[f"conv{g}_{ax}.weight"].reshape(hid, cin, 5) for g in "zrq")

        def padded(w):   # the input channels padded to eight chunks of 32
            wp = torch.zeros(w.shape[0], 256, 5)
            wp[:, :cin] = w
            return wp
        frags = torch.cat([_frags(padded(torch.cat([wz, wr])), 12, 8),    # phase 1: [chunk][tap][z 0..5, r 0..5]
                           _frags(padded(wq), 6, 8)])                     # phase 2: [chunk][tap][q 0..5]
        biases = torch.cat([weights[f"conv{g}_{ax}.bias"] for g in "zrq"])
        _same(got[a], _packed_bytes(frags, biases, precision))
