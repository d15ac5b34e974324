"""Closed loop with the whole update block on HIP, config #1 (as tests/test_gpu_gru_epe.py): the refinement loop is
CorrBlock.lookup_convc1 -> dvccorr.UpdateBlock -> dvccorr.flow_step, with nothing from raftdvc_loop inside it.

fp32: the final low-resolution flow within 1e-3 voxel EPE of the reference's flow_lo (the north-star bound).
fp16: EPE_hip <= 2 e_ref + 1e-3, e_ref the EPE of the same loop with raftdvc_loop.update_block under
torch.autocast('cuda', float16) -- the reference's own AMP update block; the factor 2 allows for a different
summation order at equal operand precision (the form and margin of test_gpu_gru_epe.py::test_closed_loop_fp16)."""
from __future__ import annotations

import pytest
import torch

import raftdvc_loop as rl
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def setup():
    import dvccorr
    g = load_golden("epe_1_8.npz")
    p = rl.load_params(DEV)
    f0, f1 = torch.from_numpy(g["fmap0"]).to(DEV), torch.from_numpy(g["fmap1"]).to(DEV)
    B, _, h, w, d = f0.shape
    return dict(g=g, p=p, f=(f0, f1), coords0=dvccorr.coords_grid_3d(B, h, w, d, DEV),
                T=tuple(int(v) for v in g["target_shape"]), net=torch.from_numpy(g["net0"]).to(DEV),
                ctx=torch.from_numpy(g["context"]).to(DEV))


def _loop(s, precision, update):
    """raft_dvc.py:440-491; update(net, context, flow, cor) -> (net, delta_flow)."""
    import dvccorr
    p, coords0 = s["p"], s["coords0"]
    blk = dvccorr.CorrBlock(*s["f"], 4, 4, precision=precision)
    coords1, net = coords0.clone(), s["net"]
    with torch.no_grad():
        for _ in range(12):
            cor = blk.lookup_convc1(coords1, p["encoder.convc1.weight"], p["encoder.convc1.bias"])
            net, delta = update(net, s["ctx"], coords1 - coords0, cor)
            coords1, _ = dvccorr.flow_step(coords1, delta, s["T"])
    torch.cuda.synchronize()
    return rl.epe(coords1 - coords0, s["g"]["flow_lo"])


def _hip(s, precision):
    import dvccorr
    blk = dvccorr.UpdateBlock(s["p"], precision=precision)
    return lambda net, ctx, flow, cor: blk(net, ctx, flow, cor=cor)[:2]


def test_closed_loop_fp32(setup):
    e = _loop(setup, "fp32", _hip(setup, "fp32"))
    print(f"EPE[hip update block fp32] = {e:.3e} voxel")
    assert e <= 1e-3, e


def test_closed_loop_fp16(setup):
    def amp(net, ctx, flow, cor):
        with torch.autocast("cuda", dtype=torch.float16):
            net, delta = rl.update_block(setup["p"], net, ctx, flow, cor=cor)
        return net.float(), delta.float()
    e_ref = _loop(setup, "fp16", amp)
    e_hip = _loop(setup, "fp16", _hip(setup, "fp16"))
    print(f"EPE[hip update block fp16] = {e_hip:.3e} voxel, EPE[autocast fp16 composition] = {e_ref:.3e} voxel")
    assert e_hip <= 2 * e_ref + 1e-3, (e_hip, e_ref)
