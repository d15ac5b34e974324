"""GPU parity of convc1 fused into the fp32 ON-THE-FLY lookup (k_fused_proj_f32 behind
dvc_corr_lookup_fused_proj with DVC_F32, CorrBlockFused(precision="fp32").lookup_convc1,
ShardedCorrBlock(precision="fp32", impl="fused").lookup_convc1).

Reference: CorrBlockOnTheFly in fp32 (src/core/corr_otf.py:96-237, the evaluation path of legacy checkpoints,
src/core/raft_dvc.py:403-412) followed by MotionEncoder's F.relu(self.convc1(corr)) (src/core/update.py:219-222,
246).  The window dots are the fp32 on-the-fly lookup's (three bf16 pieces per operand, fp32 values) and convc1
runs on bf16 hi / lo splits of both operands, so the tolerance is the fp32 one of the project,
max|out - ref| / max|ref| <= 1e-5, against the golden reference, the f64 oracle and the unfused
composition of the same block alike.
"""
from __future__ import annotations

import glob
import os

import numpy as np
import pytest
import torch

import prng
from conftest import GOLDEN, load_golden, proj_inputs
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-5
DEV = torch.device("cuda:0")
PROJ_CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "proj_*.npz")))


@pytest.fixture(scope="module", autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


def _gpu(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrs]


def _conv_inputs(seed, L, r):
    K = L * (2 * r + 1) ** 3
    bound = 1.0 / np.sqrt(K)
    return prng.uniform(seed, (96, K), -bound, bound), prng.uniform(seed + 1, (96,), -bound, bound)


def _no_composition(*a, **k):
    raise AssertionError("fp32 on-the-fly lookup_convc1 took the composition")


def _fused_block(t1, t2, L, r, legacy=False):
    """An fp32 on-the-fly block whose lookup_convc1 must run the fused kernel."""
    import dvccorr
    blk = dvccorr.CorrBlockFused(t1, t2, L, r, legacy_wd_swap=legacy, precision="fp32")
    blk._convc1_composition = _no_composition
    return blk


def _bench_like(S, C, max_flow, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    f1 = torch.randn(1, C, S, S, S, generator=g).to(DEV)
    f2 = torch.randn(1, C, S, S, S, generator=g).to(DEV)
    base = torch.stack(torch.meshgrid(*[torch.arange(S, dtype=torch.float32)] * 3, indexing="ij"))[None]
    coords = (base + (torch.rand(1, 3, S, S, S, generator=g) * 2 - 1) * max_flow).to(DEV)
    return f1, f2, coords


@pytest.mark.parametrize("case", PROJ_CASES)
def test_golden_reference_no_composition(case):
    g = load_golden(case + ".npz")
    f1, f2, coords, w, b, L, r, legacy = proj_inputs(g)
    t1, t2, tc, tw, tb = _gpu(f1, f2, coords, w, b)
    out = _fused_block(t1, t2, L, r, legacy).lookup_convc1(tc, tw, tb)
    torch.cuda.synchronize()
    assert out.shape == g["out"].shape and out.dtype == torch.float32
    err = orc.rel_err(out.cpu().numpy(), g["out"])
    print(f"{case}: rel err {err:.3e}")
    assert err < FP32_TOL


def test_direct_call_and_pack_check():
    """The C-ABI call with DVC_F32 against the f64 oracle; the single-block pack never reaches the kernel."""
    import dvccorr
    from dvccorr import ops
    H, W, D = 10, 9, 8
    C, L, r = 32, 2, 3
    f1 = prng.normal(71, (1, C, H, W, D))
    f2 = prng.normal(72, (1, C, H, W, D))
    coords = prng.flow_coords(73, 1, H, W, D, 2.0)
    w, b = _conv_inputs(74, L, r)
    ref = orc.motion_convc1(orc.corr_lookup(f1, f2, coords, L, r, False), w, b)
    t1, t2, tc, tw, tb = _gpu(f1, f2, coords, w, b)
    blk = dvccorr.CorrBlockFused(t1, t2, L, r, precision="fp32")
    out = ops.lookup_fused_proj(blk._q, blk._t, tc.reshape(1, 3, -1), ops.proj_pack(tw, L, r, False, exact=True), tb,
                                C, H, W, D, L, r, False, ops.DVC_F32)
    err = orc.rel_err(out.reshape(ref.shape).cpu().numpy(), ref)
    print(f"direct: rel err {err:.3e}")
    assert err < FP32_TOL
    with pytest.raises(ValueError, match="exact=True"):
        ops.lookup_fused_proj(blk._q, blk._t, tc.reshape(1, 3, -1), ops.proj_pack(tw, L, r, False), tb,
                              C, H, W, D, L, r, False, ops.DVC_F32)


@pytest.mark.parametrize("shape,C,L,r,legacy,B", [
    ((9, 7, 5), 32, 2, 1, False, 1),      # 315 queries: a partial last chunk, KS = 1
    ((12, 10, 16), 64, 3, 2, False, 2),   # two batch elements (one sort each), KS = 2
    ((16, 16, 16), 32, 4, 3, False, 1),
    ((8, 8, 8), 16, 4, 4, True, 1),       # level 3 = 1^3: zero level; C padded to 32
    ((10, 12, 12), 32, 2, 4, True, 1),    # legacy with W == D
    ((11, 9, 13), 128, 3, 4, False, 1),   # KS = 4, odd extents
])
def test_against_oracle(shape, C, L, r, legacy, B):
    H, W, D = shape
    seed = 2900 + H + 3 * W + 7 * D + r
    f1 = prng.normal(seed, (B, C, H, W, D))
    f2 = prng.normal(seed + 1, (B, C, H, W, D))
    coords = prng.flow_coords(seed + 2, B, H, W, D, 2.5)
    w, b = _conv_inputs(seed + 3, L, r)
    ref = orc.motion_convc1(orc.corr_lookup(f1, f2, coords, L, r, legacy), w, b)
    t1, t2, tc, tw, tb = _gpu(f1, f2, coords, w, b)
    out = _fused_block(t1, t2, L, r, legacy).lookup_convc1(tc, tw, tb)
    err = orc.rel_err(out.cpu().numpy(), ref)
    print(f"{shape} C={C} L={L} r={r}: rel err {err:.3e}")
    assert err < FP32_TOL


@pytest.mark.parametrize("S,L,max_flow", [(32, 4, 2.0), (40, 2, 6.0)])
def test_against_unfused_and_deterministic(S, L, max_flow):
    """Bench-like volumes (the #3 shape; a 40^3 L=2 one with +-6-voxel flows, whose windows spread wider than one
    origin column): fused vs relu(conv3d(blk(coords))) of the same fp32 block; bitwise repeatable."""
    C, r = 128, 4
    f1, f2, coords = _bench_like(S, C, max_flow, 277 + S)
    w, b = (torch.from_numpy(a).to(DEV) for a in _conv_inputs(278, L, r))
    blk = _fused_block(f1, f2, L, r)
    ref = torch.relu(torch.nn.functional.conv3d(blk(coords), w.view(96, -1, 1, 1, 1), b))
    out = blk.lookup_convc1(coords, w, b)
    out2 = blk.lookup_convc1(coords, w, b)
    torch.cuda.synchronize()
    err = float((out - ref).abs().max() / ref.abs().max())
    print(f"S={S} L={L}: fused vs unfused {err:.3e}")
    assert err < FP32_TOL, err
    assert torch.equal(out, out2)


def test_outliers_nonfinite_and_far_windows():
    """NaN coordinates and windows entirely outside the volume sample zeros (relu(b)); a few queries with
    +-20-voxel flows among +-1-voxel ones stay exact (they sort next to their window neighbours)."""
    H = W = D = 16
    C, L, r = 32, 2, 4
    f1 = prng.normal(61, (1, C, H, W, D))
    f2 = prng.normal(62, (1, C, H, W, D))
    coords = prng.flow_coords(63, 1, H, W, D, 1.0)
    rng = np.random.default_rng(64)
    idx = rng.integers(0, H, size=(40, 3))
    for (y, x, z) in idx:
        coords[0, :, y, x, z] += rng.uniform(-20, 20, size=3).astype(np.float32)
    coords[0, :, 1, 2, 3] = np.nan
    coords[0, 0, 4, 4, 4] = 1e30
    coords[0, :, 5, 5, 5] = -200.0      # window misses every level
    w, b = _conv_inputs(65, L, r)
    far = coords.copy()                  # the oracle takes the zero-sampling cases as far windows
    far[0, :, 1, 2, 3] = -200.0
    far[0, 0, 4, 4, 4] = -200.0
    ref = orc.motion_convc1(orc.corr_lookup(f1, f2, far, L, r, False), w, b)
    t1, t2, tc, tw, tb = _gpu(f1, f2, coords, w, b)
    out = _fused_block(t1, t2, L, r).lookup_convc1(tc, tw, tb).cpu().numpy()
    assert np.isfinite(out).all()
    relu_b = np.maximum(b, 0).astype(np.float32)
    for (y, x, z) in ((1, 2, 3), (4, 4, 4), (5, 5, 5)):
        np.testing.assert_allclose(out[0, :, y, x, z], relu_b, rtol=0, atol=1e-6)
    err = orc.rel_err(out, ref)
    print(f"outliers: rel err {err:.3e}")
    assert err < FP32_TOL


def test_repeatable_under_poisoned_memory():
    """Stale workspaces: the caching allocator is filled with -7 / 3e4 / NaN between calls, so every workspace
    the kernels get holds stale values; 6 calls (12x10x16, C=64, L=3, r=2) must all equal the first, bit for bit."""
    import dvccorr
    from dvccorr import ops
    H, W, D = 12, 10, 16
    C, L, r, B = 64, 3, 2, 1
    seed = 1900 + H + 3 * W + 7 * D + r
    f1 = prng.normal(seed, (2, C, H, W, D))[1:]
    f2 = prng.normal(seed + 1, (2, C, H, W, D))[1:]
    coords = prng.flow_coords(seed + 2, 2, H, W, D, 2.5)[1:]
    w, b = _conv_inputs(seed + 3, L, r)
    t1, t2, tc, tw, tb = _gpu(f1, f2, coords, w, b)
    nws = ops.lib().dvc_lookup_fused_proj_workspace_bytes(B, H * W * D)
    blk = dvccorr.CorrBlockFused(t1, t2, L, r, precision="fp32")
    pw = ops.proj_pack(tw, L, r, False, exact=True)

    def call(ws):
        return ops.lookup_fused_proj(blk._q, blk._t, tc.reshape(B, 3, -1), pw, tb, C, H, W, D, L, r, False,
                                     blk._dt, workspace=ws).clone()

    ref = call(torch.zeros((nws,), dtype=torch.uint8, device=DEV))
    ora = orc.motion_convc1(orc.corr_lookup(f1, f2, coords, L, r, False), w, b)
    assert orc.rel_err(ref.reshape(ora.shape).cpu().numpy(), ora) < FP32_TOL
    differ = 0
    for it in range(6):
        bufs = [torch.full((mb * (1 << 20) // 4,), (-7.0, 3.0e4, float("nan"))[it % 3], device=DEV)
                for mb in (1, 3, 7, 16, 40) for _ in range(3)]
        del bufs
        differ += not torch.equal(call(torch.empty((nws,), dtype=torch.uint8, device=DEV)), ref)
    assert differ == 0, f"{differ} of 6 calls differ"


def test_lookup_tensor_never_allocated():
    """The L (2r+1)^3-channel lookup tensor (B L (2r+1)^3 Nq 4 bytes, ~80 MB here) is gone: one lookup_convc1
    allocates the 96-channel output and the sort workspace only (~11 MB), under half of it."""
    S, C, L, r = 24, 64, 2, 4
    f1, f2, coords = _bench_like(S, C, 2.0, 301)
    w, b = (torch.from_numpy(a).to(DEV) for a in _conv_inputs(302, L, r))
    import dvccorr
    blk = dvccorr.CorrBlockFused(f1, f2, L, r, precision="fp32")
    out = blk.lookup_convc1(coords, w, b)      # warm-up: weight pack cached, kernels loaded
    del out
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = blk.lookup_convc1(coords, w, b)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - before
    lookup_bytes = 1 * L * (2 * r + 1) ** 3 * S ** 3 * 4
    print(f"peak growth {grew / 2**20:.1f} MiB; lookup tensor {lookup_bytes / 2**20:.1f} MiB")
    assert grew < lookup_bytes / 2, (grew, lookup_bytes)


def test_fallbacks_unchanged():
    """Legacy levels with W != D and radius 5 keep the composition (the direct call is refused); so does an fp32
    on-the-fly block under autograd, whose output then carries the gradient to convc1.weight."""
    import dvccorr
    from dvccorr import ops
    for (H, W, D, C, L, r, legacy) in ((8, 8, 16, 32, 2, 2, True), (8, 8, 8, 32, 2, 5, False)):
        seed = 3100 + D + r
        f1 = prng.normal(seed, (1, C, H, W, D))
        f2 = prng.normal(seed + 1, (1, C, H, W, D))
        coords = prng.flow_coords(seed + 2, 1, H, W, D, 2.0)
        w, b = _conv_inputs(seed + 3, L, r)
        ref = orc.motion_convc1(orc.corr_lookup(f1, f2, coords, L, r, legacy), w, b)
        t1, t2, tc, tw, tb = _gpu(f1, f2, coords, w, b)
        blk = dvccorr.CorrBlockFused(t1, t2, L, r, legacy_wd_swap=legacy, precision="fp32")
        out = blk.lookup_convc1(tc, tw, tb)
        err = orc.rel_err(out.cpu().numpy(), ref)
        print(f"fallback {(H, W, D)} r={r}: rel err {err:.3e}")
        assert err < FP32_TOL
        with pytest.raises(NotImplementedError):
            pw = (ops.proj_pack(tw, L, r, legacy, exact=True) if r <= 4
                  else torch.zeros((1 << 20,), dtype=torch.float16, device=DEV))
            ops.lookup_fused_proj(blk._q, blk._t, tc.reshape(1, 3, -1), pw, tb, C, H, W, D, L, r, legacy,
                                  ops.DVC_F32)

    H, W, D, C, L, r = 10, 9, 8, 32, 2, 3
    f1 = prng.normal(71, (1, C, H, W, D))
    f2 = prng.normal(72, (1, C, H, W, D))
    coords = prng.flow_coords(73, 1, H, W, D, 2.0)
    w, b = _conv_inputs(74, L, r)
    t1, t2, tc, tw, tb = _gpu(f1, f2, coords, w, b)
    blk = dvccorr.CorrBlockFused(t1, t2, L, r, precision="fp32")
    plain = blk.lookup_convc1(tc, tw, tb)
    with torch.enable_grad():
        wg = tw.clone().requires_grad_()
        out = blk.lookup_convc1(tc, wg, tb)
        assert out.grad_fn is not None
        out.sum().backward()
    assert float((out.detach() - plain).abs().max() / plain.abs().max()) < FP32_TOL
    assert wg.grad is not None and wg.grad.shape == wg.shape and bool(torch.isfinite(wg.grad).all())
    assert float(wg.grad.abs().max()) > 0


def test_sharded_fused_convc1_matches_block():
    """ShardedCorrBlock(precision="fp32", impl="fused").lookup_convc1 on one rank equals the block's."""
    from dvccorr.sharded import ShardedCorrBlock
    S, C, L, r = 24, 64, 3, 4
    f1, f2, coords = _bench_like(S, C, 2.0, 91)
    w, b = (torch.from_numpy(a).to(DEV) for a in _conv_inputs(92, L, r))
    ref = _fused_block(f1, f2, L, r).lookup_convc1(coords, w, b)
    sh = ShardedCorrBlock(f1, f2, S, L, r, precision="fp32", impl="fused")
    out = sh.lookup_convc1(coords, w, b)
    assert torch.equal(out, ref)
