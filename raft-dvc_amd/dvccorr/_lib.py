"""ctypes binding of libdvccorr.so (the C ABI declared in include/dvccorr.h).

The shared library is built in-tree (raft-dvc_amd/csrc/Makefile, or
`python -c "import __graft_entry__ as g; g.build()"`) and loaded from this
directory.  There is no fallback: if the library is missing the import of the
product path fails loudly.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DVCCORR_LIB (diagnostics): load another in-tree build of the same ABI, e.g. for A/B kernel timing
LIB_PATH = os.environ.get("DVCCORR_LIB") or os.path.join(_HERE, "libdvccorr.so")

DVC_OK, DVC_ERR_INVALID, DVC_ERR_UNSUPPORTED, DVC_ERR_LAUNCH, DVC_ERR_RUNTIME = range(5)
DVC_F32, DVC_BF16, DVC_F16 = 0, 1, 2
DVC_BRICKED = 0x100     # layout flag ORed into a dtype (include/dvccorr.h)
DVC_FIXED, DVC_LEGACY = 0, 1
MAX_LEVELS = 8

# Every symbol include/dvccorr.h declares (checked by tests/test_capi_cpu.py).
EXPORTED = (
    "dvc_layout_init", "dvc_pack_workspace_bytes", "dvc_pack_queries", "dvc_pack_targets", "dvc_pack_targets_gathered",
    "dvc_corr_build",
    "dvc_corr_pool", "dvc_corr_lookup", "dvc_lookup_fused_workspace_bytes", "dvc_corr_lookup_fused",
    "dvc_sample3d", "dvc_set_tuning", "dvc_last_error", "dvc_version", "dvc_abi_version",
    "dvc_corr_backward_workspace_bytes", "dvc_corr_backward_workspace_bytes_dtype", "dvc_corr_backward",
    "dvc_proj_packed_bytes", "dvc_proj_pack", "dvc_proj_pack_exact",
    "dvc_corr_lookup_proj", "dvc_lookup_fused_proj_workspace_bytes", "dvc_corr_lookup_fused_proj",
    "dvc_coords_grid", "dvc_upflow", "dvc_flow_step", "dvc_bricked_levels", "dvc_lookup_coarse_levels", "dvc_corr_backward_mfma", "dvc_corr_backward_gout64",
    "dvc_gru_packed_bytes", "dvc_gru_pack", "dvc_sep_gru_pass",
    "dvc_conv3_packed_bytes", "dvc_conv3_pack", "dvc_conv3",
    "dvc_conv7_flow_packed_bytes", "dvc_conv7_flow_pack", "dvc_conv7_flow",
    "dvc_conv3_pack_dgrad", "dvc_conv3_grad_prep", "dvc_conv3_wgrad_workspace_bytes", "dvc_conv3_wgrad",
    "dvc_sep_gru_pass_save", "dvc_gru_dgrad_packed_bytes", "dvc_gru_pack_dgrad", "dvc_gru_grad_prep",
    "dvc_sep_gru_dgrad", "dvc_gru_wgrad_workspace_bytes", "dvc_gru_wgrad",
    "dvc_conv7_wgrad_workspace_bytes", "dvc_conv7_wgrad",
    "dvc_enc_stem_packed_bytes", "dvc_enc_stem_pack", "dvc_enc_stem",
    "dvc_enc_conv_packed_bytes", "dvc_enc_conv_pack", "dvc_enc_conv",
    "dvc_enc_partials_bytes", "dvc_enc_stats", "dvc_enc_residual",
    "dvc_enc_grad_partials_bytes", "dvc_enc_norm_grad", "dvc_enc_grad_add", "dvc_enc_split_grad",
    "dvc_enc_dgrad_packed_bytes", "dvc_enc_conv_pack_dgrad", "dvc_enc_dgrad",
    "dvc_enc_wgrad_workspace_bytes", "dvc_enc_wgrad", "dvc_enc_stem_wgrad_workspace_bytes", "dvc_enc_stem_wgrad",
)
PROJ_COUT = 96          # DVC_PROJ_COUT (convc1 output channels, update.py:222)
PROJ_MAX_RADIUS = 4     # DVC_PROJ_MAX_RADIUS
GRU_HIDDEN = 96         # DVC_GRU_HIDDEN (SepConvGRU3D hidden channels the kernel covers, update.py:283-297)
GRU_MAX_INPUT = 160     # DVC_GRU_MAX_INPUT
GRU_SEG = 8             # DVC_GRU_SEG: output positions along the conv axis per workgroup of k_sep_gru_pass
CONV3_TH, CONV3_TW, CONV3_TD = 4, 4, 16     # DVC_CONV3_TH / TW / TD: output box of one k_conv3_mfma workgroup
CONV3_MAX_CIN = 128     # DVC_CONV3_MAX_CIN
CONV3_MAX_COUT = 128    # DVC_CONV3_MAX_COUT
# DVC_CONV3_WGRAD_KH / KW / KD: the K-block (a voxel box) of k_conv3_wgrad; DVC_CONV3_WGRAD_TARGET: the workgroups the
# slab rule aims for (ops.conv3_wgrad_slabs); DVC_CONV3_PREP_CHUNK: voxels per workgroup of k_conv3_grad_prep
CONV3_WGRAD_KH, CONV3_WGRAD_KW, CONV3_WGRAD_KD = 4, 4, 16
CONV3_WGRAD_TARGET = 512
CONV3_PREP_CHUNK = 4096
# DVC_GRU_WGRAD_LINES x DVC_GRU_WGRAD_POS: the K-block of k_gru_wgrad; DVC_GRU_WGRAD_TARGET: the workgroups its slab rule
# aims for (ops.gru_wgrad_slabs)
GRU_WGRAD_LINES, GRU_WGRAD_POS, GRU_WGRAD_TARGET = 32, 4, 512
CONV7_TH, CONV7_TW, CONV7_TD = 4, 4, 16     # DVC_CONV7_TH / TW / TD: output box of one k_conv7_flow workgroup
CONV7_COUT = 64         # DVC_CONV7_COUT (encoder.convf1, update.py:225)
# DVC_CONV7_WGRAD_KH / KW / KD: the K-block (a voxel box) of k_conv7_wgrad; DVC_CONV7_WGRAD_TILES: the 16-column tiles of
# the 1029 weight columns one workgroup owns; DVC_CONV7_WGRAD_TARGET: the workgroups its slab rule aims for
# (ops.conv7_wgrad_slabs)
CONV7_WGRAD_KH, CONV7_WGRAD_KW, CONV7_WGRAD_KD = 4, 4, 16
CONV7_WGRAD_TILES = 5
CONV7_WGRAD_TARGET = 256
# the encoders' forward (csrc/encoder.hip): DVC_ENC_TH / TW / TD the output box of one workgroup (TW is 2 for the
# strided 3 x 3 x 3 layers), DVC_ENC_STEM_COUT conv1's width, DVC_ENC_MAX_CIN / MAX_COUT the channel counts k_enc_conv
# covers (cin a multiple of 8), and the prologue / shortcut modes
ENC_TH, ENC_TW, ENC_TD = 4, 4, 16
ENC_STEM_COUT = 32
ENC_MAX_CIN, ENC_MAX_COUT = 128, 160
ENC_IDENTITY, ENC_RELU, ENC_NORM_RELU = 0, 1, 2
ENC_SC_PLAIN, ENC_SC_NORM, ENC_SC_NORM_RELU = 0, 1, 2
ENC_STEM_TAPS = 343     # the stem's `taps` in dvc_enc_partials_bytes / dvc_enc_stats
# the encoders' backward (csrc/encoder_grad.hip): DVC_ENC_GRAD_CHUNK voxels per workgroup of the norm-gradient kernels,
# DVC_ENC_WGRAD_TARGET the workgroups k_enc_wgrad's slab rule aims for
ENC_GRAD_CHUNK = 4096
ENC_WGRAD_TARGET = 1024


class Layout(ctypes.Structure):
    """Mirror of dvc_layout."""
    _fields_ = [
        ("num_levels", ctypes.c_int32),
        ("channels", ctypes.c_int32),
        ("c_pad", ctypes.c_int32),
        ("H", ctypes.c_int32 * MAX_LEVELS),
        ("W", ctypes.c_int32 * MAX_LEVELS),
        ("D", ctypes.c_int32 * MAX_LEVELS),
        ("Dp", ctypes.c_int32 * MAX_LEVELS),
        ("zero_level", ctypes.c_int32 * MAX_LEVELS),
        ("offset", ctypes.c_int64 * MAX_LEVELS),
        ("level_elems", ctypes.c_int64 * MAX_LEVELS),
        ("row_elems", ctypes.c_int64),
        ("row_stride", ctypes.c_int64),
    ]

    def levels(self):
        return [(self.H[l], self.W[l], self.D[l]) for l in range(self.num_levels)]


class DvcError(RuntimeError):
    """A HIP launch/runtime failure reported by libdvccorr."""


_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `make -C raft-dvc_amd/csrc` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = ctypes.CDLL(LIB_PATH)
    i32, i64, vp, sz = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
    sig = {
        "dvc_layout_init": (i32, [i32, i32, i32, i32, i32, ctypes.POINTER(Layout)]),
        "dvc_bricked_levels": (i32, [ctypes.POINTER(Layout)]),
        "dvc_lookup_coarse_levels": (i32, [i32, ctypes.c_int64, i32, i32, i32, i32, i32, i32, i32]),
        "dvc_pack_workspace_bytes": (sz, [i32, i32, i32, i32, i32, i32]),
        "dvc_pack_queries": (i32, [vp, vp, i32, i32, i64, i32, vp]),
        "dvc_pack_targets": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
        "dvc_pack_targets_gathered": (i32, [vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
        "dvc_corr_build": (i32, [vp, vp, vp, i32, i64, i32, i32, i32, i32, i32, i32, i32, i64, i64, vp]),
        "dvc_corr_pool": (i32, [vp, i32, i64, i32, i32, i32, i32, i32, i32, vp]),
        "dvc_corr_lookup": (i32, [vp, vp, vp, i32, i64, i32, i32, i32, i32, i32, i32, i32, vp]),
        "dvc_lookup_fused_workspace_bytes": (sz, [i32, i64, i32, i32]),
        "dvc_corr_lookup_fused": (i32, [vp, vp, vp, vp, vp, i32, i64, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
        "dvc_sample3d": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i64, i32, vp]),
        "dvc_corr_backward_workspace_bytes": (sz, [i32, i64, i32, i32, i32, i32, i32, i32]),
        "dvc_corr_backward_workspace_bytes_dtype": (sz, [i32, i64, i32, i32, i32, i32, i32, i32, i32]),
        "dvc_corr_backward": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i64, i32, i32, i32, i32, i32, i32, i32, i32,
                                    vp]),
        "dvc_corr_backward_mfma": (i32, [i32, i64, i32, i32, i32, i32, i32, i32, i32, i32]),
        "dvc_corr_backward_gout64": (i32, [i64, i32]),
        "dvc_proj_packed_bytes": (sz, [i32, i32]),
        "dvc_proj_pack": (i32, [vp, vp, i32, i32, i32, i32, vp]),
        "dvc_proj_pack_exact": (i32, [vp, vp, i32, i32, i32, i32, vp]),
        "dvc_corr_lookup_proj": (i32, [vp, vp, vp, vp, vp, i32, i64, i32, i32, i32, i32, i32, i32, i32, vp]),
        "dvc_lookup_fused_proj_workspace_bytes": (sz, [i32, i64]),
        "dvc_corr_lookup_fused_proj": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i64, i32, i32, i32, i32, i32, i32, i32,
                                             i32, vp]),
        "dvc_coords_grid": (i32, [vp, i32, i32, i32, i32, vp]),
        "dvc_upflow": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
        "dvc_flow_step": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
        "dvc_gru_packed_bytes": (sz, [i32, i32, i32]),
        "dvc_gru_pack": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
        "dvc_sep_gru_pass": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
        "dvc_conv3_packed_bytes": (sz, [i32, i32, i32]),
        "dvc_conv3_pack": (i32, [vp, vp, vp, i32, i32, i32, vp]),
        "dvc_conv3": (i32, [vp, i32, vp, i32, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
        "dvc_conv3_pack_dgrad": (i32, [vp, vp, i32, i32, i32, vp]),
        "dvc_conv3_grad_prep": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
        "dvc_conv3_wgrad_workspace_bytes": (sz, [i32, i32, i32, i32, i32, i32]),
        "dvc_conv3_wgrad": (i32, [vp, i32, vp, i32, vp, i32, vp, vp, i32, i32, i32, i32, i32, vp]),
        "dvc_sep_gru_pass_save": (i32, [vp] * 5 + [i32] * 8 + [vp]),
        "dvc_gru_dgrad_packed_bytes": (sz, [i32, i32, i32]),
        "dvc_gru_pack_dgrad": (i32, [vp, vp, vp, vp, i32, i32, i32, vp]),
        "dvc_gru_grad_prep": (i32, [vp] * 10 + [i32] * 5 + [vp]),
        "dvc_sep_gru_dgrad": (i32, [vp] * 10 + [i32] * 9 + [vp]),
        "dvc_gru_wgrad_workspace_bytes": (sz, [i32] * 7),
        "dvc_gru_wgrad": (i32, [vp] * 8 + [i32] * 8 + [vp]),
        "dvc_conv7_flow_packed_bytes": (sz, [i32]),
        "dvc_conv7_flow_pack": (i32, [vp, vp, vp, i32, vp]),
        "dvc_conv7_flow": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp]),
        "dvc_conv7_wgrad_workspace_bytes": (sz, [i32, i32, i32, i32]),
        "dvc_conv7_wgrad": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
        "dvc_enc_stem_packed_bytes": (sz, [i32]),
        "dvc_enc_stem_pack": (i32, [vp, vp, vp, i32, vp]),
        "dvc_enc_stem": (i32, [vp, vp, vp, vp] + [i32] * 6 + [vp]),
        "dvc_enc_conv_packed_bytes": (sz, [i32, i32, i32, i32]),
        "dvc_enc_conv_pack": (i32, [vp, vp, vp, i32, i32, i32, i32, vp]),
        "dvc_enc_conv": (i32, [vp, vp, i32, vp, vp, vp, i32, vp] + [i32] * 9 + [vp]),
        "dvc_enc_partials_bytes": (sz, [i32] * 7),
        "dvc_enc_stats": (i32, [vp, vp] + [i32] * 7 + [ctypes.c_float, vp]),
        "dvc_enc_residual": (i32, [vp, vp, vp, vp, i32, vp] + [i32] * 5 + [vp]),
        "dvc_enc_grad_partials_bytes": (sz, [i32] * 5),
        "dvc_enc_norm_grad": (i32, [vp, vp, vp, i32, vp, vp, vp] + [i32] * 5 + [vp]),
        "dvc_enc_grad_add": (i32, [vp, vp, vp, vp, ctypes.c_longlong, vp]),
        "dvc_enc_split_grad": (i32, [vp] * 5 + [i32] * 6 + [vp]),
        "dvc_enc_dgrad_packed_bytes": (sz, [i32] * 4),
        "dvc_enc_conv_pack_dgrad": (i32, [vp, vp] + [i32] * 4 + [vp]),
        "dvc_enc_dgrad": (i32, [vp, vp, vp] + [i32] * 9 + [vp]),
        "dvc_enc_wgrad_workspace_bytes": (sz, [i32] * 8),
        "dvc_enc_wgrad": (i32, [vp, vp, i32, vp, vp, vp] + [i32] * 9 + [vp]),
        "dvc_enc_stem_wgrad_workspace_bytes": (sz, [i32] * 5),
        "dvc_enc_stem_wgrad": (i32, [vp, vp, vp, vp] + [i32] * 6 + [vp]),
        "dvc_set_tuning": (i32, [ctypes.c_char_p, i32]),
        "dvc_last_error": (ctypes.c_char_p, []),
        "dvc_version": (ctypes.c_char_p, []),
        "dvc_abi_version": (i32, []),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _lib = L
    return L


def check(rc: int, what: str = "") -> None:
    """Turn a dvc_status into the exception the reference would raise."""
    if rc == DVC_OK:
        return
    msg = lib().dvc_last_error().decode(errors="replace")
    if what:
        msg = f"{what}: {msg}"
    if rc == DVC_ERR_INVALID:
        raise ValueError(msg)
    if rc == DVC_ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise DvcError(msg)


def set_tuning(key: str, value: int) -> None:
    check(lib().dvc_set_tuning(key.encode(), int(value)), "set_tuning")


def layout(H: int, W: int, D: int, num_levels: int, C: int = 1) -> Layout:
    """Pyramid geometry.  Raises RuntimeError where the reference's avg_pool3d would."""
    lay = Layout()
    rc = lib().dvc_layout_init(H, W, D, num_levels, C, ctypes.byref(lay))
    if rc != DVC_OK:
        raise RuntimeError(lib().dvc_last_error().decode(errors="replace"))
    return lay


def lookup_coarse_levels(B: int, Nq: int, H: int, W: int, D: int, num_levels: int, radius: int, legacy: bool,
                         store_dtype: int) -> int:
    """Trailing levels that dvc_corr_lookup with these arguments stages whole in LDS under the current tuning."""
    return int(lib().dvc_lookup_coarse_levels(B, Nq, H, W, D, num_levels, radius, 1 if legacy else 0, store_dtype))


def bricked_levels(lay: Layout) -> int:
    """Bit mask of the levels a DVC_BRICKED pyramid stores in (1, 8, 8) bricks."""
    return int(lib().dvc_bricked_levels(ctypes.byref(lay)))
