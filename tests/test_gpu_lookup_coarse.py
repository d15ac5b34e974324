"""The coarse-level path of the tile lookup (csrc/lookup_coarse.h, tuning "lookup_coarse"): small levels staged whole
in LDS instead of plane by plane.  Every comparison is bitwise: lookup_coarse on (1 = the default: the coarse levels as
one unit per tile, dispatched first; 2 - 4 = one unit per level and / or dispatched last) against lookup_coarse 0 and
against the lane-per-query walk (lookup_variant 0 on a linear block), under every dispatch shape the launch takes at these
sizes.  The path is carried by the 16-bit instances of radius <= 4; test_eligibility asserts, through the launch's own
rule (dvc_lookup_coarse_levels), which levels take it."""
from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DEFAULTS = {"lookup_coarse": 1, "lookup_variant": 2, "split_tiles": 1024, "split_ach": 5}
# one workgroup walks all levels (the coarse path declines); level split with the 5-row split; level split alone
DISPATCH = ({"split_tiles": 0}, {"split_ach": 5}, {"split_ach": 0})
COARSE = (1, 2, 3, 4)


@pytest.fixture(scope="module", autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


def _reset(_lib):
    for k, v in DEFAULTS.items():
        _lib.set_tuning(k, v)


def _inputs(B, shape, r, seed):
    import dvccorr
    H, W, D = shape
    g = torch.Generator(device="cpu").manual_seed(seed)
    f1 = torch.randn(B, 32, H, W, D, generator=g).to(DEV)
    f2 = torch.randn(B, 32, H, W, D, generator=g).to(DEV)
    base = dvccorr.coords_grid_3d(B, H, W, D, torch.device("cpu"))
    # windows leave the volume on every side; one NaN, one huge and one -inf coordinate
    wide = base + (torch.rand(B, 3, H, W, D, generator=g) * 2 - 1) * (r + 6)
    flat = wide[0].view(3, -1)
    flat[:, 5] = float("nan")
    flat[1, 17] = 1e30
    flat[2, 23] = -float("inf")
    return f1, f2, (wide.to(DEV), base.clone().to(DEV))   # (wide flow, all-zero flow)


def _check_block(f1, f2, coords, L, r, prec, legacy, tag):
    import dvccorr
    from dvccorr import _lib
    lin = dvccorr.CorrBlock(f1, f2, L, r, legacy_wd_swap=legacy, precision=prec, bricked=False)
    blk = dvccorr.CorrBlock(f1, f2, L, r, legacy_wd_swap=legacy, precision=prec)
    for ci, c in enumerate(coords):
        _lib.set_tuning("lookup_variant", 0)
        walk = lin(c)
        _lib.set_tuning("lookup_variant", 2)
        for disp in DISPATCH:
            _reset(_lib)
            for k, v in disp.items():
                _lib.set_tuning(k, v)
            _lib.set_tuning("lookup_coarse", 0)
            plain = blk(c)
            assert torch.equal(plain, walk), (tag, prec, legacy, ci, disp, "lookup_coarse 0 vs walk")
            for mode in COARSE:
                _lib.set_tuning("lookup_coarse", mode)
                for b in (blk, lin):
                    out = b(c)
                    assert torch.equal(out, plain), (tag, prec, legacy, ci, disp, mode, "vs lookup_coarse 0",
                                                     float((out - plain).abs().nan_to_num(1e30).max()))
                    assert torch.equal(out, walk), (tag, prec, legacy, ci, disp, mode, "vs walk")


# (16,16,16) L 4: levels 16 / 8 / 4 / 2 -- three coarse levels of a 16-bit pyramid, the 2^3 one narrower than every
# window; (12,20,8) L 3: non-cubic, D halves to 2 (Dp padding), every legacy level has W != D (generic: the coarse
# path declines); (6,10,12) L 2: Nq % 64 != 0, a ragged last tile, also with B = 2
@pytest.mark.parametrize("r", [1, 4, 6])
@pytest.mark.parametrize("shape,L,B", [((16, 16, 16), 4, 1), ((12, 20, 8), 3, 1), ((6, 10, 12), 2, 1),
                                       ((6, 10, 12), 2, 2)])
def test_coarse_matches_tile_and_walk(shape, L, B, r):
    from dvccorr import _lib
    f1, f2, coords = _inputs(B, shape, r, shape[0] * 1000 + shape[1] * 10 + shape[2] + r + 77 * B)
    try:
        for prec in ("bf16", "fp16", "fp32"):
            for legacy in (False, True):
                _check_block(f1, f2, coords, L, r, prec, legacy, (shape, L, B, r))
    finally:
        _reset(_lib)


# (shape, L, r, precision, legacy, B, Nq or None = the whole volume) -> trailing levels staged whole.  By hand from the
# rule: H_l W_l Dp_l esz <= 1024 bytes (r = 3, 4), 256 (r = 1, 2); 16-bit pyramids of r <= 4 only; not a
# zero, generic (legacy, W != D) or bricked level; level-split launches only.
ELIGIBLE = [
    (((16, 16, 16), 4, 4, "bf16", False, 1, None), 3),    # 8^3 = 1024 bytes exactly, 4^3, 2^3
    (((16, 16, 16), 4, 4, "fp16", False, 1, None), 3),
    (((16, 16, 16), 4, 4, "fp32", False, 1, None), 0),    # the fp32 instances do not carry the path
    (((16, 16, 16), 4, 1, "bf16", False, 1, None), 2),    # r = 1: 256 bytes -- 4^3 (4 x 4 x Dp 8 x 2) and 2^3
    (((16, 16, 16), 4, 6, "bf16", False, 1, None), 0),    # r = 6 instances do not carry it
    (((16, 16, 16), 2, 4, "bf16", False, 1, None), 1),    # budget edge: the 8^3 level, 64 KB of rows per tile
    (((16, 16, 16), 2, 4, "fp32", False, 1, None), 0),    # 128 KB: keeps the plane pipeline
    (((12, 20, 8), 3, 4, "bf16", False, 1, None), 2),     # (6, 10, Dp 8) = 960 bytes and (3, 5, Dp 8)
    (((12, 20, 8), 3, 4, "bf16", True, 1, None), 0),      # legacy, W != D at every level: generic
    (((6, 10, 12), 2, 4, "bf16", False, 2, None), 1),     # (3, 5, Dp 8) = 240 bytes; level 0 is 1920
    (((16, 16, 16), 4, 4, "bf16", False, 1, 203), 3),     # a slab of rows
    (((32, 32, 32), 4, 4, "bf16", False, 1, None), 2),    # the benchmark's launch: levels 2 (8^3) and 3 (4^3)
]


@pytest.mark.parametrize("case,expect", ELIGIBLE)
def test_eligibility(case, expect):
    """Which levels the launch stages whole, asked of the library's own launch rule: a host bug that left the coarse
    path unused (or took it where it must decline) would pass every bitwise comparison above."""
    from dvccorr import _lib, ops
    from dvccorr.corr_block import brick_flag
    (H, W, D), L, r, prec, legacy, B, nq = case
    ldt = ops.dtype_code(prec) | brick_flag(ops.layout(H, W, D, L, 32), r, legacy, True)
    args = (B, nq or H * W * D, H, W, D, L, r, legacy, ldt)
    try:
        _reset(_lib)
        assert _lib.lookup_coarse_levels(*args) == expect
        for mode in COARSE:
            _lib.set_tuning("lookup_coarse", mode)
            assert _lib.lookup_coarse_levels(*args) == expect, mode
        _lib.set_tuning("lookup_coarse", 0)
        assert _lib.lookup_coarse_levels(*args) == 0
        _reset(_lib)
        _lib.set_tuning("split_tiles", 0)      # one workgroup walks every level: the path declines
        assert _lib.lookup_coarse_levels(*args) == 0
        _reset(_lib)
        _lib.set_tuning("lookup_variant", 0)   # the walk
        assert _lib.lookup_coarse_levels(*args) == 0
    finally:
        _reset(_lib)


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_budget_edge(prec):
    """An 8^3 last level: exactly 64 KB of rows per tile for a bf16 pyramid (eligible), 128 KB for an fp32 one (the
    level keeps the plane pipeline).  Either way the outputs are those of lookup_coarse 0 and of the walk."""
    from dvccorr import _lib
    f1, f2, coords = _inputs(1, (16, 16, 16), 4, 4242)
    try:
        _check_block(f1, f2, coords, 2, 4, prec, False, ("budget", prec))
    finally:
        _reset(_lib)


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_slab(prec):
    """A rank's slab of query rows (neither its start nor its length a multiple of 64) through dvc_corr_lookup, as
    the sharded path calls it: the rows' own pyramid and coordinates."""
    import dvccorr
    from dvccorr import _lib, ops
    H, W, D, L, r = 16, 16, 16, 4, 4
    q0, nq = 37, 203
    f1, f2, coords = _inputs(1, (H, W, D), r, 99)
    c = coords[0].reshape(1, 3, -1)[:, :, q0:q0 + nq].contiguous()
    try:
        lin = dvccorr.CorrBlock(f1, f2, L, r, precision=prec, bricked=False)
        blk = dvccorr.CorrBlock(f1, f2, L, r, precision=prec)
        _lib.set_tuning("lookup_variant", 0)
        walk = ops.lookup(lin._corr[:, q0:q0 + nq].contiguous(), c, H, W, D, L, r, False, lin._ldt)
        _lib.set_tuning("lookup_variant", 2)
        rows = blk._corr[:, q0:q0 + nq].contiguous()
        outs = {}
        for mode in (0,) + COARSE:
            _lib.set_tuning("lookup_coarse", mode)
            outs[mode] = ops.lookup(rows, c, H, W, D, L, r, False, blk._ldt)
        for mode in COARSE:
            assert torch.equal(outs[mode], outs[0]), (prec, mode, "vs lookup_coarse 0")
            assert torch.equal(outs[mode], walk), (prec, mode, "vs walk")
        # the same rows inside the whole volume's lookup
        _lib.set_tuning("lookup_coarse", 1)
        whole = blk(coords[0]).reshape(1, -1, H * W * D)[:, :, q0:q0 + nq]
        assert torch.equal(whole, outs[1]), prec
    finally:
        _reset(_lib)
