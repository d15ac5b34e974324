"""CPU: the argument checks of convf1's weight gradient (dvc_conv7_wgrad), of dvccorr.conv7x7x7_flow_ad and of
dvccorr.update_block_ad run without a GPU."""
from __future__ import annotations

import ctypes
import os
import re

import pytest
import torch

import update_cases as uc
from conftest import REPO


def test_library_constants_match_header():
    from dvccorr import _lib
    txt = open(os.path.join(REPO, "include", "dvccorr.h")).read()
    for macro, val in (("DVC_CONV7_WGRAD_KH", _lib.CONV7_WGRAD_KH), ("DVC_CONV7_WGRAD_KW", _lib.CONV7_WGRAD_KW),
                       ("DVC_CONV7_WGRAD_KD", _lib.CONV7_WGRAD_KD), ("DVC_CONV7_WGRAD_TILES", _lib.CONV7_WGRAD_TILES),
                       ("DVC_CONV7_WGRAD_TARGET", _lib.CONV7_WGRAD_TARGET)):
        assert int(re.search(rf"#define {macro} (\d+)", txt).group(1)) == val
    for sym in ("dvc_conv7_wgrad", "dvc_conv7_wgrad_workspace_bytes"):
        assert sym in _lib.EXPORTED and sym in txt


def test_c_entry_points_reject_bad_arguments():
    from dvccorr import _lib, ops
    L = _lib.lib()
    F32, INV, UNS = _lib.DVC_F32, _lib.DVC_ERR_INVALID, _lib.DVC_ERR_UNSUPPORTED
    flow = ctypes.c_void_p(4096)
    g = ctypes.c_void_p(1 << 34)
    dw = ctypes.c_void_p(1 << 40)     # far from the inputs: no overlap
    ws = ctypes.c_void_p(1 << 44)
    vol = (1, 4, 4, 4)
    # dvc_conv7_wgrad(flow, g, dw, workspace, B, H, W, D, dtype, stream)
    assert L.dvc_conv7_wgrad(None, g, dw, ws, *vol, F32, None) == INV
    with pytest.raises(ValueError, match="null pointer"):
        _lib.check(INV)
    assert L.dvc_conv7_wgrad(flow, None, dw, ws, *vol, F32, None) == INV
    assert L.dvc_conv7_wgrad(flow, g, None, ws, *vol, F32, None) == INV
    assert L.dvc_conv7_wgrad(flow, g, dw, None, *vol, F32, None) == INV
    assert L.dvc_conv7_wgrad(flow, g, dw, ws, 1, 4, 0, 4, F32, None) == INV          # empty volume
    assert L.dvc_conv7_wgrad(flow, g, dw, ws, 0, 4, 4, 4, F32, None) == INV
    assert L.dvc_conv7_wgrad(flow, g, dw, ws, *vol, 7, None) == INV                   # dtype
    rc = L.dvc_conv7_wgrad(flow, g, flow, ws, *vol, F32, None)                        # dw is flow
    assert rc == INV
    with pytest.raises(ValueError, match="overlap"):
        _lib.check(rc)
    assert L.dvc_conv7_wgrad(flow, g, g, ws, *vol, F32, None) == INV                  # dw is g
    assert L.dvc_conv7_wgrad(flow, g, dw, g, *vol, F32, None) == INV                  # workspace is g
    assert L.dvc_conv7_wgrad(flow, g, dw, flow, *vol, F32, None) == INV               # workspace is flow
    assert L.dvc_conv7_wgrad(flow, g, dw, dw, *vol, F32, None) == INV                 # workspace is dw
    inside = ctypes.c_void_p((1 << 34) + 64 * 64 * 4 - 4)                             # the last float of g
    assert L.dvc_conv7_wgrad(flow, g, inside, ws, *vol, F32, None) == INV
    assert L.dvc_conv7_wgrad(flow, g, dw, ws, 2, 1024, 1024, 1024, F32, None) == UNS  # 2^31 voxels
    # the workspace: slabs x 64 x 1029 floats, the slab rule of include/dvccorr.h (ops.conv7_wgrad_slabs)
    groups = -(-65 // _lib.CONV7_WGRAD_TILES)
    for shape in ((1, 32, 32, 32), (2, 5, 9, 7), (1, 3, 3, 3), (1, 20, 28, 16), (1, 1, 1, 1), (3, 7, 5, 33),
                  (1, 3, 3, 23 * 16 - 5)):
        nbox, per, nslab = ops.conv7_wgrad_slabs(*shape)
        assert (nslab - 1) * per < nbox <= nslab * per                                # no empty slab
        assert nslab <= -(-_lib.CONV7_WGRAD_TARGET // groups)
        assert L.dvc_conv7_wgrad_workspace_bytes(*shape) == nslab * 64 * 1029 * 4
    assert ops.conv7_wgrad_slabs(1, 32, 32, 32) == (128, 7, 19)
    for shape in ((1, 4, 0, 4), (0, 4, 4, 4), (2, 1024, 1024, 1024)):
        assert L.dvc_conv7_wgrad_workspace_bytes(*shape) == 0


def test_fake_shapes():
    import dvccorr.library  # noqa: F401
    flow, g = torch.empty(2, 3, 5, 9, 7, device="meta"), torch.empty(2, 64, 5, 9, 7, device="meta")
    w, b = torch.empty(64, 3, 7, 7, 7, device="meta"), torch.empty(64, device="meta")
    for dt in (0, 1, 2):
        dw = torch.ops.dvccorr.conv7_wgrad(flow, g, dt)
        assert tuple(dw.shape) == (64, 3, 7, 7, 7) and dw.dtype == torch.float32
        y = torch.ops.dvccorr.conv7_ad(flow, w, b, dt)
        assert tuple(y.shape) == (2, 64, 5, 9, 7) and y.dtype == torch.float32


def test_conv7_validation_without_gpu():
    import dvccorr
    p = uc.params("upd_215")
    w, b = p["encoder.convf1.weight"], p["encoder.convf1.bias"]
    flow = torch.zeros(1, 3, 4, 4, 4)
    with pytest.raises(ValueError, match=r"\(3, 4, 4, 4\)"):
        dvccorr.conv7x7x7_flow_ad(flow[0], w, b)
    with pytest.raises(ValueError, match="do not match"):
        dvccorr.conv7x7x7_flow_ad(flow[:, :2], w, b)
    with pytest.raises(ValueError, match="do not match"):
        dvccorr.conv7x7x7_flow_ad(flow, w, b[:5])
    with pytest.raises(ValueError, match="do not match"):
        dvccorr.conv7x7x7_flow_ad(flow, p["encoder.convf2.weight"], b)       # a 3 x 3 x 3 weight
    with pytest.raises(RuntimeError, match="MI355X"):
        dvccorr.conv7x7x7_flow_ad(flow, w, b)
    with pytest.raises(RuntimeError, match="MI355X"):                        # also where grad is asked for
        dvccorr.conv7x7x7_flow_ad(flow, w.clone().requires_grad_(True), b)


def test_update_block_validation_without_gpu():
    import dvccorr
    p = uc.params("upd_215")
    vol = (2, 1, 5)
    net, ctx, flow = torch.zeros(1, 96, *vol), torch.zeros(1, 64, *vol), torch.zeros(1, 3, *vol)
    cor = torch.zeros(1, 96, *vol)
    with pytest.raises(ValueError, match="exactly one"):
        dvccorr.update_block_ad(net, ctx, flow, p)
    with pytest.raises(ValueError, match="exactly one"):
        dvccorr.update_block_ad(net, ctx, flow, p, cor=cor, corr=cor)
    with pytest.raises(ValueError, match="missing weights"):
        dvccorr.update_block_ad(net, ctx, flow, {n: t for n, t in p.items() if n != "flow_head.conv2.bias"}, cor=cor)
    with pytest.raises(ValueError, match=r"\(96, 2, 1, 5\)"):
        dvccorr.update_block_ad(net[0], ctx, flow, p, cor=cor)
    with pytest.raises(ValueError, match="differ"):
        dvccorr.update_block_ad(net, ctx, flow, p, cor=torch.zeros(1, 96, 2, 1, 6))
    with pytest.raises(ValueError, match="3 channels"):
        dvccorr.update_block_ad(net, ctx, torch.zeros(1, 2, *vol), p, cor=cor)
    with pytest.raises(ValueError, match="3 channels"):
        dvccorr.update_block_ad(net, ctx, flow, p, cor=cor[:, :95])
    with pytest.raises(RuntimeError, match="MI355X"):
        dvccorr.update_block_ad(net, ctx, flow, p, cor=cor)
    with pytest.raises(RuntimeError, match="MI355X"):                        # requires-grad inputs are accepted
        dvccorr.update_block_ad(net.clone().requires_grad_(True), ctx, flow, p, cor=cor)


def test_exported_names():
    import dvccorr
    for name in ("conv7x7x7_flow_ad", "update_block_ad"):
        assert name in dvccorr.__all__ and name in dvccorr.update.__all__ and callable(getattr(dvccorr, name))
    import dvccorr.library as library
    assert "conv7_ad" in library.__all__ and "conv7_wgrad" in library.__all__
