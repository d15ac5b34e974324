"""Closed loop with the HIP GRU, config #1 (as tests/test_gpu_epe.py): dvccorr's CorrBlock, flow_step and
SepConvGRU inside the reference's refinement loop; the motion encoder and the flow head come from raftdvc_loop, the
GRU weights from epe_meta.json.

fp32: the final low-resolution flow within 1e-3 voxel EPE of the reference's flow_lo (the north-star bound).
fp16: EPE_hip <= 2 e_ref + 1e-3, e_ref the EPE of the same loop with raftdvc_loop.sep_gru under
torch.autocast('cuda', float16) -- the reference's own AMP GRU; the factor 2 allows for a different summation order
at equal operand precision."""
from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

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
    return dict(g=g, p=p, blk=dvccorr.CorrBlock(f0, f1, 4, 4, precision="fp32"),
                coords0=dvccorr.coords_grid_3d(B, h, w, d, DEV), T=tuple(int(v) for v in g["target_shape"]),
                net=torch.from_numpy(g["net0"]).to(DEV), ctx=torch.from_numpy(g["context"]).to(DEV))


def _loop(s, gru_fn):
    """raftdvc_loop.refine with the GRU pluggable (update.py:338-342)."""
    import dvccorr
    p, coords0 = s["p"], s["coords0"]
    coords1, net = coords0.clone(), s["net"]
    with torch.no_grad():
        for _ in range(12):
            corr = s["blk"](coords1)
            flow = coords1 - coords0
            inp = torch.cat([s["ctx"], rl.motion_features(p, flow, corr)], dim=1)
            net = gru_fn(net, inp)
            delta = rl._conv(p, "flow_head.conv2", F.relu(rl._conv(p, "flow_head.conv1", net, 1)), 1)
            coords1, _ = dvccorr.flow_step(coords1, delta, s["T"])
    torch.cuda.synchronize()
    return rl.epe(coords1 - coords0, s["g"]["flow_lo"])


def _hip_gru(s, precision):
    import dvccorr
    return dvccorr.SepConvGRU({n[4:]: t for n, t in s["p"].items() if n.startswith("gru.")}, precision=precision)


def test_closed_loop_fp32(setup):
    e = _loop(setup, _hip_gru(setup, "fp32"))
    print(f"EPE[hip gru fp32] = {e:.3e} voxel")
    assert e <= 1e-3, e


def test_closed_loop_fp16(setup):
    def amp_gru(net, inp):
        with torch.autocast("cuda", dtype=torch.float16):
            return rl.sep_gru(setup["p"], net, inp).float()
    e_ref = _loop(setup, amp_gru)
    e_hip = _loop(setup, _hip_gru(setup, "fp16"))
    print(f"EPE[hip gru fp16] = {e_hip:.3e} voxel, EPE[autocast fp16 composition] = {e_ref:.3e} voxel")
    assert e_hip <= 2 * e_ref + 1e-3, (e_hip, e_ref)
