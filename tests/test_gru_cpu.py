"""CPU: the SepConvGRU checker is pinned on the reference's fixtures, and the argument checks of
dvccorr.sep_conv_gru / SepConvGRU and of the two C entry points run without a GPU."""
from __future__ import annotations

import ctypes
import os
import re

import pytest
import torch

import gru_cases as gc
from conftest import REPO


@pytest.mark.parametrize("name", gc.CASES)
def test_checker_reproduces_reference_passes(name):
    """raftdvc_loop.sep_gru (and its per-pass restriction) against the reference's h after each pass: <= 1e-6."""
    p = gc.params()
    h, x, ref = gc.inputs(name)
    with torch.no_grad():
        got = gc.checker_passes(p, h, x)
        end = gc.checker(p, h, x)
    for ax, a, r in zip(gc.AXES, got, ref):
        e = gc.err(a, r)
        print(f"{name} pass {ax}: {e:.2e}")
        assert e <= 1e-6, (name, ax, e)
    assert gc.err(end, ref[2]) <= 1e-6


def test_library_constants_match_header():
    from dvccorr import _lib
    txt = open(os.path.join(REPO, "include", "dvccorr.h")).read()
    for macro, val in (("DVC_GRU_SEG", _lib.GRU_SEG), ("DVC_GRU_HIDDEN", _lib.GRU_HIDDEN),
                       ("DVC_GRU_MAX_INPUT", _lib.GRU_MAX_INPUT)):
        assert int(re.search(rf"#define {macro} (\d+)", txt).group(1)) == val
    assert "dvc_gru_pack" in _lib.EXPORTED and "dvc_sep_gru_pass" in _lib.EXPORTED


def test_python_validation_without_gpu():
    import dvccorr
    p = gc.params()
    h, x = torch.zeros(1, 96, 4, 4, 4), torch.zeros(1, 147, 4, 4, 4)
    with pytest.raises(ValueError, match=r"\(96, 4, 4, 4\)"):            # not 5-D
        dvccorr.sep_conv_gru(h[0], x, p)
    with pytest.raises(ValueError, match="differ"):                       # batch
        dvccorr.sep_conv_gru(h, torch.zeros(2, 147, 4, 4, 4), p)
    with pytest.raises(ValueError, match="differ"):                       # spatial
        dvccorr.sep_conv_gru(h, torch.zeros(1, 147, 4, 4, 5), p)
    with pytest.raises(ValueError, match="do not match"):                 # channels against the weights
        dvccorr.sep_conv_gru(h, torch.zeros(1, 146, 4, 4, 4), p)
    with pytest.raises(ValueError, match="do not match"):
        dvccorr.sep_conv_gru(torch.zeros(1, 95, 4, 4, 4), x, p)
    short = {k: v for k, v in p.items() if k != "convq_d.bias"}
    with pytest.raises(ValueError, match="convq_d.bias"):
        dvccorr.sep_conv_gru(h, x, short)
    with pytest.raises(ValueError, match="convq_d.bias"):
        dvccorr.SepConvGRU(short)
    with pytest.raises(RuntimeError, match="MI355X"):                     # CPU tensors are refused
        dvccorr.sep_conv_gru(h, x, p)
    with pytest.raises(RuntimeError, match="MI355X"):
        dvccorr.SepConvGRU(p)(h, x)


def test_c_entry_points_reject_bad_arguments():
    from dvccorr import _lib
    L = _lib.lib()
    a = ctypes.c_void_p(4096)
    b = ctypes.c_void_p(1 << 40)     # far from a: no overlap
    ok = (1, 96, 147, 4, 4, 4)
    assert L.dvc_sep_gru_pass(None, a, a, b, *ok, 0, _lib.DVC_F32, None) == _lib.DVC_ERR_INVALID
    with pytest.raises(ValueError, match="null pointer"):
        _lib.check(_lib.DVC_ERR_INVALID)
    assert L.dvc_sep_gru_pass(a, a, None, b, *ok, 0, _lib.DVC_F32, None) == _lib.DVC_ERR_INVALID
    assert L.dvc_sep_gru_pass(a, a, a, None, *ok, 0, _lib.DVC_F32, None) == _lib.DVC_ERR_INVALID
    for axis in (-1, 3):
        assert L.dvc_sep_gru_pass(a, a, a, b, *ok, axis, _lib.DVC_F32, None) == _lib.DVC_ERR_INVALID
    assert L.dvc_sep_gru_pass(a, a, a, b, 1, 96, 147, 0, 4, 4, 0, _lib.DVC_F32, None) == _lib.DVC_ERR_INVALID
    assert L.dvc_sep_gru_pass(a, a, a, b, *ok, 0, 7, None) == _lib.DVC_ERR_INVALID                    # dtype
    assert L.dvc_sep_gru_pass(a, a, a, a, *ok, 0, _lib.DVC_F32, None) == _lib.DVC_ERR_INVALID         # h_out is h
    rc = L.dvc_sep_gru_pass(a, a, a, b, 1, 32, 147, 4, 4, 4, 0, _lib.DVC_F32, None)
    assert rc == _lib.DVC_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError, match="hidden=32"):
        _lib.check(rc)
    assert L.dvc_sep_gru_pass(a, a, a, b, 1, 96, 161, 4, 4, 4, 0, _lib.DVC_F32, None) == _lib.DVC_ERR_UNSUPPORTED
    assert L.dvc_gru_pack(None, a, a, a, a, a, a, 96, 147, _lib.DVC_F32, None) == _lib.DVC_ERR_INVALID
    assert L.dvc_gru_pack(a, a, a, a, a, a, None, 96, 147, _lib.DVC_F32, None) == _lib.DVC_ERR_INVALID
    assert L.dvc_gru_pack(a, a, a, a, a, a, a, 64, 147, _lib.DVC_F32, None) == _lib.DVC_ERR_UNSUPPORTED
    assert L.dvc_gru_pack(a, a, a, a, a, a, a, 96, 147, 9, None) == _lib.DVC_ERR_INVALID
    # one axis: 720 one-KB fragments per piece (two pieces for fp32) and 288 biases
    assert L.dvc_gru_packed_bytes(96, 147, _lib.DVC_BF16) == 720 * 1024 + 288 * 4
    assert L.dvc_gru_packed_bytes(96, 147, _lib.DVC_F32) == 2 * 720 * 1024 + 288 * 4
    assert L.dvc_gru_packed_bytes(32, 19, _lib.DVC_F32) == 0
