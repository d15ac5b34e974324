"""CPU: the argument checks of the conv3x3x3 backward's C entry points and of dvccorr.conv3x3x3_ad run without a GPU."""
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
    for macro, val in (("DVC_CONV3_WGRAD_KH", _lib.CONV3_WGRAD_KH), ("DVC_CONV3_WGRAD_KW", _lib.CONV3_WGRAD_KW),
                       ("DVC_CONV3_WGRAD_KD", _lib.CONV3_WGRAD_KD), ("DVC_CONV3_WGRAD_TARGET", _lib.CONV3_WGRAD_TARGET),
                       ("DVC_CONV3_PREP_CHUNK", _lib.CONV3_PREP_CHUNK)):
        assert int(re.search(rf"#define {macro} (\d+)", txt).group(1)) == val
    for sym in ("dvc_conv3_pack_dgrad", "dvc_conv3_grad_prep", "dvc_conv3_wgrad", "dvc_conv3_wgrad_workspace_bytes"):
        assert sym in _lib.EXPORTED and sym in txt


def test_c_entry_points_reject_bad_arguments():
    from dvccorr import _lib, ops
    L = _lib.lib()
    F32, BF16, INV, UNS = _lib.DVC_F32, _lib.DVC_BF16, _lib.DVC_ERR_INVALID, _lib.DVC_ERR_UNSUPPORTED
    a = ctypes.c_void_p(4096)
    a2 = ctypes.c_void_p(1 << 30)
    g = ctypes.c_void_p(1 << 34)
    b = ctypes.c_void_p(1 << 40)     # far from the inputs: no overlap
    ws = ctypes.c_void_p(1 << 44)
    vol = (1, 4, 4, 4)
    # dvc_conv3_wgrad(src0, c0, src1, c1, g, cout, dw, workspace, B, H, W, D, dtype, stream)
    assert L.dvc_conv3_wgrad(None, 96, a2, 32, g, 80, b, ws, *vol, F32, None) == INV
    with pytest.raises(ValueError, match="null pointer"):
        _lib.check(INV)
    assert L.dvc_conv3_wgrad(a, 96, a2, 32, None, 80, b, ws, *vol, F32, None) == INV
    assert L.dvc_conv3_wgrad(a, 96, a2, 32, g, 80, None, ws, *vol, F32, None) == INV
    assert L.dvc_conv3_wgrad(a, 96, a2, 32, g, 80, b, None, *vol, F32, None) == INV
    assert L.dvc_conv3_wgrad(a, 96, a2, 32, g, 80, b, ws, 1, 4, 0, 4, F32, None) == INV          # empty volume
    assert L.dvc_conv3_wgrad(a, 96, a2, 32, g, 80, b, ws, *vol, 7, None) == INV                   # dtype
    rc = L.dvc_conv3_wgrad(a, 96, a2, 32, g, 80, a, ws, *vol, F32, None)                          # dw is src0
    assert rc == INV
    with pytest.raises(ValueError, match="overlap"):
        _lib.check(rc)
    assert L.dvc_conv3_wgrad(a, 96, a2, 32, g, 80, a2, ws, *vol, F32, None) == INV                # dw is src1
    assert L.dvc_conv3_wgrad(a, 96, a2, 32, g, 80, g, ws, *vol, F32, None) == INV                 # dw is g
    assert L.dvc_conv3_wgrad(a, 96, a2, 32, g, 80, b, g, *vol, F32, None) == INV                  # workspace is g
    assert L.dvc_conv3_wgrad(a, 96, a2, 32, g, 80, b, b, *vol, F32, None) == INV                  # workspace is dw
    assert L.dvc_conv3_wgrad(a, 0, None, 0, g, 80, b, ws, *vol, F32, None) == INV                 # cin = 0
    assert L.dvc_conv3_wgrad(a, 96, None, 0, g, 0, b, ws, *vol, F32, None) == INV                 # cout = 0
    rc = L.dvc_conv3_wgrad(a, 96, a2, 33, g, 80, b, ws, *vol, F32, None)                          # cin = 129
    assert rc == UNS
    with pytest.raises(NotImplementedError, match="cin=129"):
        _lib.check(rc)
    assert L.dvc_conv3_wgrad(a, 129, None, 0, g, 80, b, ws, *vol, F32, None) == UNS
    assert L.dvc_conv3_wgrad(a, 96, None, 0, g, 129, b, ws, *vol, F32, None) == UNS
    # dvc_conv3_pack_dgrad(w, packed, cin, cout, dtype, stream)
    assert L.dvc_conv3_pack_dgrad(None, a, 128, 80, F32, None) == INV
    assert L.dvc_conv3_pack_dgrad(a, None, 128, 80, F32, None) == INV
    assert L.dvc_conv3_pack_dgrad(a, b, 128, 80, 9, None) == INV
    assert L.dvc_conv3_pack_dgrad(a, b, 0, 80, F32, None) == INV
    assert L.dvc_conv3_pack_dgrad(a, b, 128, 0, F32, None) == INV
    rc = L.dvc_conv3_pack_dgrad(a, b, 129, 80, F32, None)
    assert rc == UNS
    with pytest.raises(NotImplementedError, match="cin=129"):
        _lib.check(rc)
    assert L.dvc_conv3_pack_dgrad(a, b, 128, 129, F32, None) == UNS
    # dvc_conv3_grad_prep(grad_y, y_or_null, g_or_null, db, partial, cout, B, H, W, D, stream)
    db, part = ctypes.c_void_p(1 << 41), ctypes.c_void_p(1 << 42)
    assert L.dvc_conv3_grad_prep(None, a2, g, db, part, 80, *vol, None) == INV
    assert L.dvc_conv3_grad_prep(a, a2, g, None, part, 80, *vol, None) == INV
    assert L.dvc_conv3_grad_prep(a, a2, g, db, None, 80, *vol, None) == INV
    assert L.dvc_conv3_grad_prep(a, a2, None, db, part, 80, *vol, None) == INV                    # y without g
    assert L.dvc_conv3_grad_prep(a, None, g, db, part, 80, *vol, None) == INV                     # g without y
    assert L.dvc_conv3_grad_prep(a, a2, a, db, part, 80, *vol, None) == INV                       # g is grad_y
    assert L.dvc_conv3_grad_prep(a, a2, a2, db, part, 80, *vol, None) == INV                      # g is y
    assert L.dvc_conv3_grad_prep(a, a2, g, db, part, 80, 1, 0, 4, 4, None) == INV                 # empty volume
    assert L.dvc_conv3_grad_prep(a, a2, g, db, part, 0, *vol, None) == INV
    assert L.dvc_conv3_grad_prep(a, a2, g, db, part, 129, *vol, None) == UNS
    # the workspace: slabs x cout x cin x 27 floats, the slab rule of include/dvccorr.h (ops.conv3_wgrad_slabs)
    for (cin, cout), shape in {(128, 80): (1, 32, 32, 32), (96, 128): (2, 5, 9, 7), (128, 3): (1, 3, 3, 3),
                               (64, 32): (1, 20, 28, 16), (1, 1): (1, 1, 1, 1)}.items():
        nbox, per, nslab = ops.conv3_wgrad_slabs(cin, cout, *shape)
        assert (nslab - 1) * per < nbox <= nslab * per                                           # no empty slab
        assert L.dvc_conv3_wgrad_workspace_bytes(cin, cout, *shape) == nslab * cout * cin * 27 * 4
    assert ops.conv3_wgrad_slabs(128, 80, 1, 32, 32, 32) == (128, 6, 22)
    assert L.dvc_conv3_wgrad_workspace_bytes(128, 80, 1, 32, 32, 32) == 22 * 80 * 128 * 27 * 4
    for cin, cout, shape in ((129, 80, vol), (128, 129, vol), (0, 80, vol), (128, 0, vol), (128, 80, (1, 4, 0, 4))):
        assert L.dvc_conv3_wgrad_workspace_bytes(cin, cout, *shape) == 0
    # the input gradient's pack is a layer with the channel counts swapped
    for cin, cout in ((128, 80), (96, 128), (128, 3), (33, 17)):
        for dt in (F32, BF16, _lib.DVC_F16):
            tiles, chunks = {128: 8, 96: 8, 33: 4}[cin], (cout + 31) // 32
            assert L.dvc_conv3_packed_bytes(cout, cin, dt) == chunks * 27 * tiles * (2 if dt == F32 else 1) * 1024 \
                + 64 * tiles


def test_dgrad_pack_fake_size_matches_library():
    """The meta implementation of dvccorr::conv3_pack_dgrad restates dvc_conv3_packed_bytes(cout, cin, dtype)."""
    from dvccorr import _lib
    import dvccorr.library  # noqa: F401
    for cout, cin in ((80, 128), (128, 96), (3, 128), (17, 33), (1, 1), (32, 64), (21, 59)):
        for dt in (0, 1, 2):
            w = torch.empty(cout, cin, 3, 3, 3, device="meta")
            got = torch.ops.dvccorr.conv3_pack_dgrad(w, dt)
            assert got.numel() * 4 == _lib.lib().dvc_conv3_packed_bytes(cout, cin, dt)


def test_python_validation_without_gpu():
    import dvccorr
    p = uc.params("upd_215")
    w, b = p["encoder.convf2.weight"], p["encoder.convf2.bias"]
    x = torch.zeros(1, 64, 4, 4, 4)
    with pytest.raises(ValueError, match=r"\(64, 4, 4, 4\)"):
        dvccorr.conv3x3x3_ad(x[0], w, b)
    with pytest.raises(ValueError, match="differ"):
        dvccorr.conv3x3x3_ad(x[:, :32], w, b, x2=torch.zeros(1, 32, 4, 4, 5))
    with pytest.raises(ValueError, match="do not match"):
        dvccorr.conv3x3x3_ad(x[:, :63], w, b)
    with pytest.raises(ValueError, match="do not match"):
        dvccorr.conv3x3x3_ad(x, w, b[:5])
    with pytest.raises(RuntimeError, match="MI355X"):
        dvccorr.conv3x3x3_ad(x, w, b)
    with pytest.raises(RuntimeError, match="MI355X"):                      # also where grad is asked for
        dvccorr.conv3x3x3_ad(x.clone().requires_grad_(True), w, b, relu=True)
    with pytest.raises(TypeError):                                         # no slice writes under autograd
        dvccorr.conv3x3x3_ad(x, w, b, out=torch.zeros(1, 32, 4, 4, 4))
