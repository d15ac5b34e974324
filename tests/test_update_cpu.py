"""CPU: the update-block checker is pinned on the reference's fixtures, and the argument checks of
dvccorr.UpdateBlock / conv3x3x3 and of the convolutions' C entry points run without a GPU."""
from __future__ import annotations

import ctypes
import os
import re

import pytest
import torch

import update_cases as uc
from conftest import REPO


@pytest.mark.parametrize("name", uc.CASES)
def test_checker_reproduces_reference_activations(name):
    """Every stored activation from the stored input of its layer, and the whole block from the inputs: <= 1e-6."""
    p, c = uc.params(name), uc.case(name)
    with torch.no_grad():
        cor = torch.relu(uc.rl._conv(p, "encoder.convc1", c["corr"], 0))
        errs = {"cor": uc.err(cor, c["cor"])}
        for layer in uc.layers_of(name):
            errs[layer] = uc.err(uc.check_layer(p, layer, *uc.layer_inputs(c, layer)), c[uc.LAYERS[layer][1]])
        mf = uc.rl.motion_features(p, c["flow"], cor=c["cor"])
        errs["motion_features"] = uc.err(mf, c["motion_features"])
        net, delta, log_b = uc.checker(p, c["net0"], c["context"], c["flow"], corr=c["corr"])
        errs["net"], errs["delta_flow"] = uc.err(net, c["net"]), uc.err(delta, c["delta_flow"])
        if "log_b" in c:
            errs["log_b"] = uc.err(log_b, c["log_b"])
            assert log_b.shape[1] == 4
        else:
            assert log_b is None
    print(name, {k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) <= 1e-6, errs


def test_library_constants_match_header():
    from dvccorr import _lib
    txt = open(os.path.join(REPO, "include", "dvccorr.h")).read()
    for macro, val in (("DVC_CONV3_TH", _lib.CONV3_TH), ("DVC_CONV3_TW", _lib.CONV3_TW),
                       ("DVC_CONV3_TD", _lib.CONV3_TD), ("DVC_CONV3_MAX_CIN", _lib.CONV3_MAX_CIN),
                       ("DVC_CONV3_MAX_COUT", _lib.CONV3_MAX_COUT), ("DVC_CONV7_TH", _lib.CONV7_TH),
                       ("DVC_CONV7_TW", _lib.CONV7_TW), ("DVC_CONV7_TD", _lib.CONV7_TD),
                       ("DVC_CONV7_COUT", _lib.CONV7_COUT)):
        assert int(re.search(rf"#define {macro} (\d+)", txt).group(1)) == val
    for sym in ("dvc_conv3_packed_bytes", "dvc_conv3_pack", "dvc_conv3", "dvc_conv7_flow_packed_bytes",
                "dvc_conv7_flow_pack", "dvc_conv7_flow"):
        assert sym in _lib.EXPORTED and sym in txt


def test_python_validation_without_gpu():
    import dvccorr
    p = uc.params("upd_215")
    net, ctx = torch.zeros(1, 96, 4, 4, 4), torch.zeros(1, 64, 4, 4, 4)
    flow, cor = torch.zeros(1, 3, 4, 4, 4), torch.zeros(1, 96, 4, 4, 4)
    blk = dvccorr.UpdateBlock(p)
    assert blk.has_uncertainty and blk.separable
    with pytest.raises(ValueError, match=r"\(96, 4, 4, 4\)"):            # not 5-D
        blk(net[0], ctx, flow, cor=cor)
    with pytest.raises(ValueError, match="differ"):                       # batch
        blk(net, torch.zeros(2, 64, 4, 4, 4), flow, cor=cor)
    with pytest.raises(ValueError, match="differ"):                       # spatial
        blk(net, ctx, torch.zeros(1, 3, 4, 4, 5), cor=cor)
    with pytest.raises(ValueError, match="3 channels"):
        blk(net, ctx, torch.zeros(1, 2, 4, 4, 4), cor=cor)
    with pytest.raises(ValueError, match="exactly one"):
        blk(net, ctx, flow)
    with pytest.raises(ValueError, match="exactly one"):
        blk(net, ctx, flow, cor=cor, corr=torch.zeros(1, 2916, 4, 4, 4))
    short = {k: v for k, v in p.items() if k != "flow_head.conv2.bias"}
    with pytest.raises(ValueError, match="flow_head.conv2.bias"):
        dvccorr.UpdateBlock(short)
    short = {k: v for k, v in p.items() if k != "uncertainty_head.conv1.weight"}
    with pytest.raises(ValueError, match="uncertainty_head.conv1.weight"):
        dvccorr.UpdateBlock(short)
    with pytest.raises(RuntimeError, match="MI355X"):                     # CPU tensors are refused
        blk(net, ctx, flow, cor=cor)
    w, b = p["encoder.convf2.weight"], p["encoder.convf2.bias"]
    x = torch.zeros(1, 64, 4, 4, 4)
    with pytest.raises(ValueError, match=r"\(64, 4, 4, 4\)"):
        dvccorr.conv3x3x3(x[0], w, b)
    with pytest.raises(ValueError, match="differ"):
        dvccorr.conv3x3x3(x[:, :32], w, b, x2=torch.zeros(1, 32, 4, 4, 5))
    with pytest.raises(ValueError, match="do not match"):
        dvccorr.conv3x3x3(x[:, :63], w, b)
    with pytest.raises(ValueError, match="not inside"):
        dvccorr.conv3x3x3(x, w, b, out=torch.zeros(1, 40, 4, 4, 4), out_offset=9)
    with pytest.raises(RuntimeError, match="MI355X"):
        dvccorr.conv3x3x3(x, w, b)


def test_c_entry_points_reject_bad_arguments():
    from dvccorr import _lib
    L = _lib.lib()
    F32, BF16, INV, UNS = _lib.DVC_F32, _lib.DVC_BF16, _lib.DVC_ERR_INVALID, _lib.DVC_ERR_UNSUPPORTED
    a = ctypes.c_void_p(4096)
    a2 = ctypes.c_void_p(1 << 30)
    b = ctypes.c_void_p(1 << 40)     # far from a and a2: no overlap
    vol = (1, 4, 4, 4)
    # dvc_conv3(src0, c0, src1, c1, packed, dst, dst_channels, dst_offset, cout, relu, B, H, W, D, dtype, stream)
    assert L.dvc_conv3(None, 96, a2, 32, a, b, 147, 64, 80, 1, *vol, F32, None) == INV
    with pytest.raises(ValueError, match="null pointer"):
        _lib.check(INV)
    assert L.dvc_conv3(a, 96, a2, 32, None, b, 147, 64, 80, 1, *vol, F32, None) == INV
    assert L.dvc_conv3(a, 96, a2, 32, a, None, 147, 64, 80, 1, *vol, F32, None) == INV
    assert L.dvc_conv3(a, 96, a2, 32, a, b, 147, 64, 80, 1, 1, 4, 0, 4, F32, None) == INV          # empty volume
    assert L.dvc_conv3(a, 96, a2, 32, a, b, 147, 64, 80, 1, *vol, 7, None) == INV                   # dtype
    assert L.dvc_conv3(a, 96, a2, 32, a, a, 147, 64, 80, 1, *vol, F32, None) == INV                 # dst is src0
    assert L.dvc_conv3(a, 96, a2, 32, a, a2, 147, 64, 80, 1, *vol, F32, None) == INV                # dst is src1
    rc = L.dvc_conv3(a, 96, a2, 32, a, b, 147, 68, 80, 1, *vol, F32, None)                          # 68 + 80 > 147
    assert rc == INV
    with pytest.raises(ValueError, match="not inside"):
        _lib.check(rc)
    assert L.dvc_conv3(a, 96, a2, 32, a, b, 147, -1, 80, 1, *vol, F32, None) == INV
    rc = L.dvc_conv3(a, 96, a2, 33, a, b, 147, 64, 80, 1, *vol, F32, None)                          # cin = 129
    assert rc == UNS
    with pytest.raises(NotImplementedError, match="cin=129"):
        _lib.check(rc)
    assert L.dvc_conv3(a, 129, None, 0, a, b, 147, 64, 80, 1, *vol, F32, None) == UNS
    assert L.dvc_conv3(a, 96, None, 0, a, b, 147, 0, 129, 1, *vol, F32, None) == UNS
    assert L.dvc_conv3_pack(None, a, a, 128, 80, F32, None) == INV
    assert L.dvc_conv3_pack(a, a, None, 128, 80, F32, None) == INV
    assert L.dvc_conv3_pack(a, a, a, 128, 80, 9, None) == INV
    assert L.dvc_conv3_pack(a, a, a, 129, 80, F32, None) == UNS
    assert L.dvc_conv7_flow(None, a, b, *vol, F32, None) == INV
    assert L.dvc_conv7_flow(a, a, None, *vol, F32, None) == INV
    assert L.dvc_conv7_flow(a, a, a, *vol, F32, None) == INV                                        # dst is flow
    assert L.dvc_conv7_flow(a, a, b, 1, 0, 4, 4, F32, None) == INV
    assert L.dvc_conv7_flow(a, a, b, *vol, 5, None) == INV
    assert L.dvc_conv7_flow_pack(a, None, a, F32, None) == INV
    assert L.dvc_conv7_flow_pack(a, a, a, 4, None) == INV
    # packed bytes: 1 KB fragments [32-channel chunk][27 taps][tile] per piece (two pieces for fp32), then 16 float32
    # biases per tile; tiles = cout / 16 rounded up to 1, 2, 4, 5 or 8
    for (cin, cout), (chunks, tiles) in {(128, 80): (4, 5), (96, 128): (3, 8), (128, 3): (4, 1)}.items():
        frag = chunks * 27 * tiles * 1024
        assert L.dvc_conv3_packed_bytes(cin, cout, BF16) == frag + 64 * tiles
        assert L.dvc_conv3_packed_bytes(cin, cout, _lib.DVC_F16) == frag + 64 * tiles
        assert L.dvc_conv3_packed_bytes(cin, cout, F32) == 2 * frag + 64 * tiles
    assert L.dvc_conv3_packed_bytes(128, 80, BF16) == 553280 and L.dvc_conv3_packed_bytes(128, 3, F32) == 221248
    assert L.dvc_conv3_packed_bytes(64, 48, BF16) == 2 * 27 * 4 * 1024 + 256      # three tiles run as four
    for cin, cout, dt in ((129, 80, F32), (128, 129, F32), (0, 80, F32), (128, 0, BF16), (128, 80, 7)):
        assert L.dvc_conv3_packed_bytes(cin, cout, dt) == 0
    # convf1: [49 (kh, kw) steps][4 tiles] fragments per piece, then 64 biases
    assert L.dvc_conv7_flow_packed_bytes(BF16) == 49 * 4 * 1024 + 256
    assert L.dvc_conv7_flow_packed_bytes(F32) == 2 * 49 * 4 * 1024 + 256
    assert L.dvc_conv7_flow_packed_bytes(3) == 0
