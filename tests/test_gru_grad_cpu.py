"""CPU: the argument checks of the GRU backward's C entry points and of dvccorr.sep_conv_gru_ad run without a GPU."""
from __future__ import annotations

import ctypes
import os
import re

import pytest
import torch

import gru_cases
from conftest import REPO

NEW = ("dvc_sep_gru_pass_save", "dvc_gru_dgrad_packed_bytes", "dvc_gru_pack_dgrad", "dvc_gru_grad_prep",
       "dvc_sep_gru_dgrad", "dvc_gru_wgrad_workspace_bytes", "dvc_gru_wgrad")


def test_library_constants_match_header():
    from dvccorr import _lib
    txt = open(os.path.join(REPO, "include", "dvccorr.h")).read()
    for macro, val in (("DVC_GRU_WGRAD_LINES", _lib.GRU_WGRAD_LINES), ("DVC_GRU_WGRAD_POS", _lib.GRU_WGRAD_POS),
                       ("DVC_GRU_WGRAD_TARGET", _lib.GRU_WGRAD_TARGET), ("DVC_GRU_SEG", _lib.GRU_SEG)):
        assert int(re.search(rf"#define {macro} (\d+)", txt).group(1)) == val
    for sym in NEW:
        assert sym in _lib.EXPORTED and sym in txt
        assert hasattr(_lib.lib(), sym)


def _ptrs(n):
    """n fake device pointers, far apart: no two buffers of the small test volume overlap"""
    return [ctypes.c_void_p((i + 1) << 34) for i in range(n)]


def test_c_entry_points_reject_bad_arguments():
    from dvccorr import _lib
    L = _lib.lib()
    F32, INV, UNS = _lib.DVC_F32, _lib.DVC_ERR_INVALID, _lib.DVC_ERR_UNSUPPORTED
    vol = (4, 4, 4)

    def sweep(fn, nptr, tail, optional=(), outputs=(), shape_at=1):
        """tail(B, hidden, input?, H, W, D, ..) as a list; every null pointer, an empty volume and every output aliasing
        another buffer is DVC_ERR_INVALID; hidden 95 is DVC_ERR_UNSUPPORTED.  Every call here is rejected before any
        launch: the pointers are fake."""
        p = _ptrs(nptr)
        for i in range(nptr):
            if i in optional:   # a valid call: it would launch on these fake pointers where there is a GPU
                continue
            q = list(p)
            q[i] = None
            rc = fn(*q, *tail, None)
            assert rc == INV, (fn.__name__, i)
            with pytest.raises(ValueError, match="null pointer"):
                _lib.check(rc)
        for o in outputs:
            for j in range(nptr):
                if j == o:
                    continue
                q = list(p)
                q[o] = p[j]
                rc = fn(*q, *tail, None)
                assert rc == INV, (fn.__name__, o, j)
                with pytest.raises(ValueError, match="overlap"):
                    _lib.check(rc)
        t = list(tail)
        t[0] = 0                                                     # B = 0
        assert fn(*p, *t, None) == INV
        t = list(tail)
        t[shape_at] = 95                                             # hidden
        rc = fn(*p, *t, None)
        assert rc == UNS
        with pytest.raises(NotImplementedError, match="hidden=95"):
            _lib.check(rc)
        return p

    # dvc_sep_gru_pass_save(h, x, packed, h_out, save, B, hidden, input, H, W, D, axis, dtype, stream)
    p = sweep(L.dvc_sep_gru_pass_save, 5, [1, 96, 147, *vol, 0, F32], outputs=(3, 4))
    assert L.dvc_sep_gru_pass_save(*p, 1, 96, 147, *vol, 3, F32, None) == INV          # axis
    assert L.dvc_sep_gru_pass_save(*p, 1, 96, 147, *vol, 0, 7, None) == INV            # dtype
    assert L.dvc_sep_gru_pass_save(*p, 1, 96, 161, *vol, 0, F32, None) == UNS
    assert L.dvc_sep_gru_pass_save(*p, 1, 96, 0, *vol, 0, F32, None) == UNS
    # dvc_gru_pack_dgrad(wz, wr, wq, packed, hidden, input, dtype, stream)
    p = _ptrs(4)
    for i in range(4):
        q = list(p)
        q[i] = None
        assert L.dvc_gru_pack_dgrad(*q, 96, 147, F32, None) == INV
    assert L.dvc_gru_pack_dgrad(*p, 96, 147, 9, None) == INV
    assert L.dvc_gru_pack_dgrad(*p, 95, 147, F32, None) == UNS
    assert L.dvc_gru_pack_dgrad(*p, 96, 161, F32, None) == UNS
    # dvc_gru_grad_prep(g, z, q, h, a_q, a_z, dh, db_q, db_z, partial, B, hidden, H, W, D, stream)
    sweep(L.dvc_gru_grad_prep, 10, [1, 96, *vol], outputs=(4, 5, 6, 7, 8, 9))
    # dvc_sep_gru_dgrad(a_q, a_z, h, r, packed, a_r, dh, dx, db_r, partial, B, hidden, input, H, W, D, axis, dx_add,
    #                   dtype, stream)
    p = sweep(L.dvc_sep_gru_dgrad, 10, [1, 96, 147, *vol, 1, 0, F32], optional=(7,), outputs=(5, 6, 7, 8, 9))
    assert L.dvc_sep_gru_dgrad(*p, 1, 96, 147, *vol, -1, 0, F32, None) == INV
    assert L.dvc_sep_gru_dgrad(*p, 1, 96, 147, *vol, 1, 0, 5, None) == INV
    assert L.dvc_sep_gru_dgrad(*p, 1, 96, 161, *vol, 1, 0, F32, None) == UNS
    # dvc_gru_wgrad(h, x, r, a_z, a_r, a_q, dw, workspace, B, hidden, input, H, W, D, axis, dtype, stream)
    p = sweep(L.dvc_gru_wgrad, 8, [1, 96, 147, *vol, 2, F32], outputs=(6, 7))
    assert L.dvc_gru_wgrad(*p, 1, 96, 147, *vol, 3, F32, None) == INV
    assert L.dvc_gru_wgrad(*p, 1, 96, 147, *vol, 2, 4, None) == INV
    assert L.dvc_gru_wgrad(*p, 1, 96, 0, *vol, 2, F32, None) == UNS


def test_byte_formulas():
    from dvccorr import _lib, ops
    L = _lib.lib()
    for dt, pieces in ((_lib.DVC_F32, 2), (_lib.DVC_BF16, 1), (_lib.DVC_F16, 1)):
        for inp in (1, 33, 147, 160):
            assert L.dvc_gru_dgrad_packed_bytes(96, inp, dt) == (3 + 6) * 5 * 16 * pieces * 1024
    for bad in ((95, 147, 0), (96, 0, 0), (96, 161, 0), (96, 147, 7)):
        assert L.dvc_gru_dgrad_packed_bytes(*bad) == 0
    for inp, shape in ((147, (1, 32, 32, 32)), (147, (2, 5, 9, 7)), (1, (1, 1, 1, 1)), (160, (1, 3, 4, 19)),
                       (33, (1, 20, 28, 16))):
        for axis in range(3):
            nkb, per, nslab = ops.gru_wgrad_slabs(inp, *shape, axis)
            assert (nslab - 1) * per < nkb <= nslab * per                                       # no empty slab
            assert L.dvc_gru_wgrad_workspace_bytes(96, inp, *shape, axis) == nslab * 3 * 96 * (96 + inp) * 5 * 4
    assert ops.gru_wgrad_slabs(147, 1, 32, 32, 32, 0) == (256, 24, 11)
    for bad in ((95, 147, 1, 4, 4, 4, 0), (96, 161, 1, 4, 4, 4, 0), (96, 147, 1, 4, 0, 4, 0), (96, 147, 1, 4, 4, 4, 3)):
        assert L.dvc_gru_wgrad_workspace_bytes(*bad) == 0


def test_fake_implementations_match_library():
    from dvccorr import _lib
    import dvccorr.library  # noqa: F401
    p = gru_cases.params()
    ws = [torch.empty(p[n].shape, device="meta") for n in gru_cases_names()]
    for dt in (0, 1, 2):
        got = torch.ops.dvccorr.gru_pack_dgrad(ws, dt)
        assert got.numel() * 4 == 3 * _lib.lib().dvc_gru_dgrad_packed_bytes(96, 147, dt)
    h, x = torch.empty(2, 96, 3, 4, 5, device="meta"), torch.empty(2, 147, 3, 4, 5, device="meta")
    out, saved = torch.ops.dvccorr.sep_gru_ad(h, x, ws, 0)
    assert tuple(out.shape) == tuple(h.shape) and tuple(saved.shape) == (11,) + tuple(h.shape)
    aq, az, dh, dbq, dbz = torch.ops.dvccorr.gru_grad_prep(h, h, h, h)
    assert tuple(aq.shape) == tuple(az.shape) == tuple(dh.shape) == tuple(h.shape) and tuple(dbq.shape) == (96,)
    ar, dbr = torch.ops.dvccorr.gru_dgrad(h, h, h, h, torch.empty(3, 8, device="meta"), dh, None, 0, False, 0)
    assert tuple(ar.shape) == tuple(h.shape) and tuple(dbr.shape) == (96,)
    assert tuple(torch.ops.dvccorr.gru_wgrad(h, x, h, h, h, h, 1, 0).shape) == (3, 96, 243, 5)


def gru_cases_names():
    import dvccorr
    return dvccorr.update.GRU_WEIGHT_NAMES


def test_python_validation_without_gpu():
    import dvccorr
    p = gru_cases.params()
    h, x = torch.zeros(1, 96, 2, 3, 4), torch.zeros(1, 147, 2, 3, 4)
    assert "sep_conv_gru_ad" in dvccorr.__all__ and "sep_conv_gru_ad" in dvccorr.update.__all__
    with pytest.raises(ValueError, match=r"\(96, 2, 3, 4\)"):
        dvccorr.sep_conv_gru_ad(h[0], x, p)
    with pytest.raises(ValueError, match="differ"):
        dvccorr.sep_conv_gru_ad(h, torch.zeros(1, 147, 2, 3, 5), p)
    with pytest.raises(ValueError, match="missing weights"):
        dvccorr.sep_conv_gru_ad(h, x, {n: t for n, t in p.items() if n != "convq_w.bias"})
    with pytest.raises(ValueError, match="do not match"):
        dvccorr.sep_conv_gru_ad(h, x[:, :100], p)
    with pytest.raises(RuntimeError, match="MI355X"):
        dvccorr.sep_conv_gru_ad(h, x, p)
    with pytest.raises(RuntimeError, match="MI355X"):                      # also where grad is asked for
        dvccorr.sep_conv_gru_ad(h.clone().requires_grad_(True), x, p)
    with pytest.raises(NotImplementedError, match="sep_conv_gru_ad"):      # the inference entry points keep refusing
        dvccorr.update._refuse_grad(h.clone().requires_grad_(True), x, p)
