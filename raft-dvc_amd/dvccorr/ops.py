"""Tensor-level wrappers over the C ABI.

PyTorch supplies device memory and the current HIP stream; every call goes
straight to libdvccorr.so (no CPU fallback).  Shapes follow include/dvccorr.h:

    pack_queries(fmap1_slab (B, C, Nq) f32)            -> (B, Nq, Cp)          dtype
    pack_targets(fmap2 (B, C, H, W, D) f32, L)         -> (B, row_stride, Cp)  dtype
    build(q, t, ...)                                   -> (B, Nq, row_stride)  store dtype
    pool(corr, ..., src_level)                         in place
    lookup(corr, coords (B, 3, Nq) f32, ...)           -> (B, L*(2r+1)^3, Nq)  f32
    lookup_fused(q, t, coords, ...)                    -> (B, L*(2r+1)^3, Nq)  f32
    sample3d(vol (B, C, Hv, Wv, Dv), pts (B, Nq, 3))   -> (B, C, Nq)           f32
    proj_pack(convc1 weight (96, L*(2r+1)^3) f32, ...) -> packed fp16 weights
    lookup_proj(corr, coords, packed_w, bias, ...)     -> (B, 96, Nq)          f32
    coords_grid(B, H, W, D, device)                    -> (B, 3, H, W, D)      f32
    upflow(flow (B, C, h, w, d), (H, W, D))            -> (B, C, H, W, D)      f32
    flow_step(coords1, delta (B, 3, h, w, d), (H,W,D)) -> coords1 + delta, upflow(coords1 + delta - coords0)
    gru_pack(18 SepConvGRU3D tensors, dtype)           -> packed weights of the three axis passes
    sep_gru(h (B, 96, H, W, D), x (B, Ci, H, W, D), packed, dtype) -> h after the h, w and d passes  f32
    conv3_pack(weight (Co, Ci, 3, 3, 3), bias, dtype)  -> packed weights of one 3 x 3 x 3 convolution
    conv3(src0, src1 | None, packed, dst, offset, Co, relu, dtype) -> dst[:, offset:offset + Co] written  f32
    conv7_flow_pack(weight (64, 3, 7, 7, 7), bias, dtype) / conv7_flow(flow, packed, dst, dtype)   encoder.convf1
    conv3_pack_dgrad(weight, dtype)                    -> packed weights of the layer's input gradient (run by conv3)
    conv3_grad_prep(grad_y, y | None, relu)            -> (grad_y * (y > 0), its per-channel sums db)
    conv3_wgrad(x, x2 | None, g, dtype)                -> dW (Co, Ci, 3, 3, 3)  f32
    conv7_wgrad(flow, g, dtype)                        -> dW (64, 3, 7, 7, 7)   f32   (encoder.convf1)
    sep_gru_save(h, x, packed, dtype)                  -> (h after the three passes, saved (11, B, 96, H, W, D))  f32
    gru_pack_dgrad(18 SepConvGRU3D tensors, dtype)     -> packed weights of the three passes' input gradients
    gru_grad_prep(g, z, q, h)                          -> (a_q, a_z, dh0, db_q, db_z) of one pass
    sep_gru_dgrad(a_q, a_z, h, r, packed_axis, dh, dx | None, axis, dx_add, dtype) -> (a_r, db_r); dh, dx in place
    gru_wgrad(h, x, r, a_z, a_r, a_q, axis, dtype)     -> dW (3, 96, 96 + Ci, 5) of one pass  f32
    enc_stem_pack(weight (32, 1, 7, 7, 7), bias, dtype) / enc_stem(x, packed, y, partials | None, stride, dtype)
    enc_conv_pack(weight (Co, Ci, 3 | 1, ..), bias, dtype) -> packed weights of one encoder convolution
    enc_conv(x, scale_shift | None, prologue, packed, y, y2 | None, partials | None, taps, stride, dtype) -> y  f32
    enc_partials(taps, stride, Co, B, ovol, device)    -> statistics partials buffer  f64
    enc_stats(partials, scale_shift (B, C, 2), taps, stride, ovol, eps) -> scale_shift written  f32
    enc_residual(c3, ss3 | None, shortcut, ss4 | None, mode, out) -> out = relu(norm3(c3) + shortcut)  f32
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import DVC_BF16, DVC_BRICKED, DVC_F16, DVC_F32, DVC_FIXED, DVC_LEGACY, bricked_levels, check, layout, lib


class _DtypeMap(dict):
    """dtype code -> torch dtype; a DVC_BRICKED layout flag ORed into the code is ignored."""

    def __getitem__(self, code):
        return super().__getitem__(int(code) & ~DVC_BRICKED)


_TORCH_DT = _DtypeMap({DVC_F32: torch.float32, DVC_BF16: torch.bfloat16, DVC_F16: torch.float16})


def dtype_code(precision: str) -> int:
    if precision in ("fp32", "float32", "f32"):
        return DVC_F32
    if precision in ("bf16", "bfloat16"):
        return DVC_BF16
    if precision in ("fp16", "float16", "f16", "half"):
        return DVC_F16
    raise ValueError(f"precision must be 'fp32', 'bf16' or 'fp16', got {precision!r}")


def _ptr(t: torch.Tensor) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr())


def _stream(t: torch.Tensor) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)



def _on_device(fn):
    """Run an op with its tensors' device current (torch.cuda.device), so the C ABI's launches, workspaces and
    the backward's side stream land on the GPU that owns the data even when the calling thread's current device
    is another one (a block on cuda:1 driven from a thread whose current device is 0)."""
    import functools

    @functools.wraps(fn)
    def run(*args, **kwargs):
        for a in list(args) + list(kwargs.values()):
            if isinstance(a, torch.Tensor) and a.is_cuda:
                with torch.cuda.device(a.device):
                    return fn(*args, **kwargs)
        return fn(*args, **kwargs)

    return run


def _need_cuda(*ts: torch.Tensor) -> None:
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError("dvccorr runs on the MI355X only: got a CPU tensor (no CPU fallback)")


def _mark(t: torch.Tensor, dtype: int) -> torch.Tensor:
    """Record the DVC_BRICKED layout flag next to a packed-target / pyramid buffer (the C ABI cannot tell)."""
    t._dvc_bricked = bool(int(dtype) & DVC_BRICKED)
    return t


def _expect_layout(t: torch.Tensor, dtype: int, what: str) -> None:
    """A buffer packed bricked must be read with DVC_BRICKED, and only by the entry points that take it."""
    rec = getattr(t, "_dvc_bricked", None)
    if rec is not None and rec != bool(int(dtype) & DVC_BRICKED):
        raise ValueError(f"{what}: the buffer was packed {'bricked' if rec else 'linear'} but is passed as "
                         f"{'bricked' if int(dtype) & DVC_BRICKED else 'linear'} (include/dvccorr.h, DVC_BRICKED)")


def _f32c(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).contiguous()


@_on_device
def pack_queries(fmap1_slab: torch.Tensor, dtype: int) -> torch.Tensor:
    _need_cuda(fmap1_slab)
    f = _f32c(fmap1_slab)
    B, C, Nq = f.shape
    Cp = 32 if C <= 32 else 64 if C <= 64 else (C + 127) // 128 * 128   # dvc_layout_init's c_pad
    out = torch.empty((B, Nq, Cp), dtype=_TORCH_DT[dtype], device=f.device)
    check(lib().dvc_pack_queries(_ptr(f), _ptr(out), B, C, Nq, dtype, _stream(f)), "pack_queries")
    return out


@_on_device
def pack_targets(fmap2: torch.Tensor, num_levels: int, dtype: int, out: torch.Tensor = None) -> torch.Tensor:
    """fmap2 -> packed targets of every level; dtype | DVC_BRICKED stores the bricked levels in brick order
    (the materialised build then writes a bricked pyramid, which only the tile lookups read)."""
    _need_cuda(fmap2)
    f = _f32c(fmap2)
    B, C, H, W, D = f.shape
    lay = layout(H, W, D, num_levels, C)
    if out is None:
        out = torch.empty((B, lay.row_stride, lay.c_pad), dtype=_TORCH_DT[dtype], device=f.device)
    nws = lib().dvc_pack_workspace_bytes(B, C, H, W, D, num_levels)
    ws = torch.empty((max(nws, 4) // 4,), dtype=torch.float32, device=f.device)
    check(lib().dvc_pack_targets(_ptr(f), _ptr(out), _ptr(ws), B, C, H, W, D, num_levels, dtype, _stream(f)),
          "pack_targets")
    return _mark(out, dtype)


@_on_device
def pack_targets_gathered(gathered: torch.Tensor, H: int, num_levels: int, dtype: int) -> torch.Tensor:
    """pack_targets of the fmap2 an H-slab all-gather delivers, read from its receive buffer
    gathered (world, B, C, ceil(H / world), W, D) without assembling fmap2 (dvc_pack_targets_gathered;
    sharded.all_gather_slab's buffer, slab r = slab_bounds(H, world, r), zero-padded)."""
    _need_cuda(gathered)
    if gathered.dtype != torch.float32 or not gathered.is_contiguous() or gathered.dim() != 6:
        raise ValueError("pack_targets_gathered: expected a contiguous float32 (world, B, C, maxh, W, D) buffer")
    world, B, C, maxh, W, D = gathered.shape
    if maxh != -(-H // world):
        raise ValueError(f"pack_targets_gathered: slab height {maxh} != ceil({H} / {world})")
    lay = layout(H, W, D, num_levels, C)
    out = torch.empty((B, lay.row_stride, lay.c_pad), dtype=_TORCH_DT[dtype], device=gathered.device)
    check(lib().dvc_pack_targets_gathered(_ptr(gathered), world, _ptr(out), B, C, H, W, D, num_levels, dtype,
                                          _stream(gathered)), "pack_targets_gathered")
    return _mark(out, dtype)


GUARD_BYTES = 256   # DVC_CORR_GUARD_BYTES


def alloc_corr(B: int, Nq: int, row_stride: int, store_dtype: int, device, zero: bool = False) -> torch.Tensor:
    """(B, Nq, row_stride) corr buffer with DVC_CORR_GUARD_BYTES of guard space on both sides (dvc_corr_build
    zeroes the guards; zero=True zeroes the whole buffer, for the pooled build whose build call covers only
    level 0's columns)."""
    dt = _TORCH_DT[store_dtype]
    g = GUARD_BYTES // torch.tensor([], dtype=dt).element_size()
    n = B * Nq * row_stride
    buf = (torch.zeros if zero else torch.empty)((n + 2 * g,), dtype=dt, device=device)
    return buf[g:g + n].view(B, Nq, row_stride)


@_on_device
def build(packed_q: torch.Tensor, packed_t: torch.Tensor, C: int, H: int, W: int, D: int, num_levels: int,
          in_dtype: int, store_dtype: int, col_begin: int = 0, col_end=None, out: torch.Tensor = None) -> torch.Tensor:
    _need_cuda(packed_q, packed_t)
    B, Nq, _ = packed_q.shape
    lay = layout(H, W, D, num_levels, C)
    col_end = lay.row_stride if col_end is None else col_end
    if out is None:
        out = alloc_corr(B, Nq, lay.row_stride, store_dtype, packed_q.device)
    check(lib().dvc_corr_build(_ptr(packed_q), _ptr(packed_t), _ptr(out), B, Nq, C, H, W, D, num_levels, in_dtype,
                               store_dtype, col_begin, col_end, _stream(packed_q)), "corr_build")
    # the build is layout-blind: bricked packed targets give a bricked pyramid
    out._dvc_bricked = getattr(packed_t, "_dvc_bricked", False)
    return out


@_on_device
def pool(corr: torch.Tensor, H: int, W: int, D: int, num_levels: int, src_level: int, store_dtype: int) -> None:
    _need_cuda(corr)
    _expect_layout(corr, store_dtype, "corr_pool")
    B, Nq, _ = corr.shape
    check(lib().dvc_corr_pool(_ptr(corr), B, Nq, H, W, D, num_levels, src_level, store_dtype, _stream(corr)),
          "corr_pool")


@_on_device
def lookup(corr: torch.Tensor, coords: torch.Tensor, H: int, W: int, D: int, num_levels: int, radius: int,
           legacy: bool, store_dtype: int, out: torch.Tensor = None) -> torch.Tensor:
    _need_cuda(corr, coords)
    _expect_layout(corr, store_dtype, "corr_lookup")
    B, Nq, _ = corr.shape
    c = _f32c(coords)
    n3 = (2 * radius + 1) ** 3
    if out is None:
        out = torch.empty((B, num_levels * n3, Nq), dtype=torch.float32, device=corr.device)
    check(lib().dvc_corr_lookup(_ptr(corr), _ptr(c), _ptr(out), B, Nq, H, W, D, num_levels, radius,
                                DVC_LEGACY if legacy else DVC_FIXED, store_dtype, _stream(corr)), "corr_lookup")
    return out


@_on_device
def proj_pack(weight: torch.Tensor, num_levels: int, radius: int, legacy: bool, exact: bool = False) -> torch.Tensor:
    """convc1.weight (96, L*(2r+1)^3[, 1, 1, 1]) -> the fused kernel's packed fp16 operand (dvc_proj_pack), or for
    fp32 pyramids (exact=True) its bf16 hi + lo blocks (dvc_proj_pack_exact, twice the bytes)."""
    _need_cuda(weight)
    w = _f32c(weight.detach().reshape(weight.shape[0], -1))
    nbytes = lib().dvc_proj_packed_bytes(num_levels, radius)
    if nbytes == 0:
        raise NotImplementedError(f"proj_pack: L={num_levels} r={radius} not supported (radius 1..4)")
    if w.shape[1] != num_levels * (2 * radius + 1) ** 3:
        raise ValueError(f"convc1 weight has {w.shape[1]} input channels; the lookup has "
                         f"{num_levels * (2 * radius + 1) ** 3}")
    out = torch.empty(((2 if exact else 1) * nbytes // 2,), dtype=torch.float16, device=w.device)
    fn = lib().dvc_proj_pack_exact if exact else lib().dvc_proj_pack
    check(fn(_ptr(w), _ptr(out), w.shape[0], num_levels, radius, DVC_LEGACY if legacy else DVC_FIXED, _stream(w)),
          "proj_pack")
    return out


_PACK_CACHE: dict = {}


def proj_pack_cached(weight: torch.Tensor, num_levels: int, radius: int, legacy: bool,
                     exact: bool = False) -> torch.Tensor:
    """proj_pack, re-packed only when the weight changes: the packing is once per optimiser step, not once
    per lookup.  Entries belong to the weight tensor OBJECT (a weak reference, checked on every hit, and a
    finalizer that drops the entry), plus its in-place version counter and shape, so a new weight that
    lands on a freed weight's address never reuses the old packing."""
    import weakref
    key = (id(weight), num_levels, radius, bool(legacy), bool(exact))
    hit = _PACK_CACHE.get(key)
    state = (weight._version, tuple(weight.shape), weight.device, weight.data_ptr())
    if hit is not None and hit[0]() is weight and hit[1] == state:
        return hit[2]
    packed = proj_pack(weight, num_levels, radius, legacy, exact)
    if hit is None or hit[0]() is not weight:
        weakref.finalize(weight, _PACK_CACHE.pop, key, None)
    _PACK_CACHE[key] = (weakref.ref(weight), state, packed)
    return packed


@_on_device
def lookup_proj(corr: torch.Tensor, coords: torch.Tensor, packed_w: torch.Tensor, bias: torch.Tensor, H: int, W: int,
                D: int, num_levels: int, radius: int, legacy: bool, store_dtype: int,
                out: torch.Tensor = None) -> torch.Tensor:
    """relu(convc1(lookup(coords))) -> (B, 96, Nq) f32, the lookup never written (dvc_corr_lookup_proj)."""
    _need_cuda(corr, coords, packed_w, bias)
    _expect_layout(corr, store_dtype, "corr_lookup_proj")
    B, Nq, _ = corr.shape
    c = _f32c(coords)
    b = _f32c(bias)
    if b.numel() != _lib.PROJ_COUT:
        raise ValueError(f"convc1 bias must have {_lib.PROJ_COUT} entries; got {b.numel()}")
    need = lib().dvc_proj_packed_bytes(num_levels, radius) * (2 if (int(store_dtype) & ~DVC_BRICKED) == DVC_F32 else 1)
    have = packed_w.numel() * packed_w.element_size()
    if have < need:
        raise ValueError(f"lookup_proj: packed_w holds {have} bytes; this store dtype's consumer reads {need} "
                         f"(fp32 pyramids take proj_pack(..., exact=True); include/dvccorr.h, ABI 3)")
    if out is None:
        out = torch.empty((B, _lib.PROJ_COUT, Nq), dtype=torch.float32, device=corr.device)
    check(lib().dvc_corr_lookup_proj(_ptr(corr), _ptr(c), _ptr(packed_w), _ptr(b), _ptr(out), B, Nq, H, W, D,
                                     num_levels, radius, DVC_LEGACY if legacy else DVC_FIXED, store_dtype,
                                     _stream(corr)), "corr_lookup_proj")
    return out


@_on_device
def lookup_fused_proj(packed_q: torch.Tensor, packed_t: torch.Tensor, coords: torch.Tensor, packed_w: torch.Tensor,
                      bias: torch.Tensor, C: int, H: int, W: int, D: int, num_levels: int, radius: int, legacy: bool,
                      dtype: int, out: torch.Tensor = None, workspace: torch.Tensor = None) -> torch.Tensor:
    """relu(convc1(lookup_fused(coords))) -> (B, 96, Nq) f32 on the on-the-fly path, the lookup never written
    (dvc_corr_lookup_fused_proj: queries grouped by window origin, convc1 on MFMA).  fp32 operands (DVC_F32) run
    k_fused_proj_f32, whose exact split consumer reads proj_pack(..., exact=True)'s hi + lo blocks."""
    _need_cuda(packed_q, packed_t, coords, packed_w, bias)
    _expect_layout(packed_t, dtype, "corr_lookup_fused_proj")
    B, Nq, _ = packed_q.shape
    c = _f32c(coords)
    b = _f32c(bias)
    if b.numel() != _lib.PROJ_COUT:
        raise ValueError(f"convc1 bias must have {_lib.PROJ_COUT} entries; got {b.numel()}")
    need = lib().dvc_proj_packed_bytes(num_levels, radius) * (2 if int(dtype) == DVC_F32 else 1)
    have = packed_w.numel() * packed_w.element_size()
    if have < need:
        raise ValueError(f"lookup_fused_proj: packed_w holds {have} bytes; this dtype's consumer reads {need} "
                         f"(fp32 blocks take proj_pack(..., exact=True); include/dvccorr.h, ABI 3)")
    if out is None:
        out = torch.empty((B, _lib.PROJ_COUT, Nq), dtype=torch.float32, device=packed_q.device)
    nws = lib().dvc_lookup_fused_proj_workspace_bytes(B, Nq)
    if workspace is None or workspace.numel() * workspace.element_size() < nws:
        workspace = torch.empty((max(nws, 256),), dtype=torch.uint8, device=packed_q.device)
    check(lib().dvc_corr_lookup_fused_proj(_ptr(packed_q), _ptr(packed_t), _ptr(c), _ptr(packed_w), _ptr(b), _ptr(out),
                                           _ptr(workspace), B, Nq, C, H, W, D, num_levels, radius,
                                           DVC_LEGACY if legacy else DVC_FIXED, dtype, _stream(packed_q)),
          "corr_lookup_fused_proj")
    return out


@_on_device
def lookup_fused(packed_q: torch.Tensor, packed_t: torch.Tensor, coords: torch.Tensor, C: int, H: int, W: int,
                 D: int, num_levels: int, radius: int, legacy: bool, dtype: int, out: torch.Tensor = None,
                 workspace: torch.Tensor = None) -> torch.Tensor:
    _need_cuda(packed_q, packed_t, coords)
    _expect_layout(packed_t, dtype, "corr_lookup_fused")
    B, Nq, _ = packed_q.shape
    c = _f32c(coords)
    n3 = (2 * radius + 1) ** 3
    if out is None:
        out = torch.empty((B, num_levels * n3, Nq), dtype=torch.float32, device=packed_q.device)
    nws = lib().dvc_lookup_fused_workspace_bytes(B, Nq, num_levels, radius)
    if workspace is None or workspace.numel() * workspace.element_size() < nws:
        workspace = torch.empty((max(nws, 4) // 4,), dtype=torch.float32, device=packed_q.device)
    check(lib().dvc_corr_lookup_fused(_ptr(packed_q), _ptr(packed_t), _ptr(c), _ptr(out), _ptr(workspace), B, Nq, C,
                                      H, W, D, num_levels, radius, DVC_LEGACY if legacy else DVC_FIXED, dtype,
                                      _stream(packed_q)), "corr_lookup_fused")
    return out


def fused_workspace(B: int, Nq: int, num_levels: int, radius: int, device) -> torch.Tensor:
    nws = lib().dvc_lookup_fused_workspace_bytes(B, Nq, num_levels, radius)
    return torch.empty((max(nws, 4) // 4,), dtype=torch.float32, device=device)


@_on_device
def corr_backward(packed_q: torch.Tensor, packed_t: torch.Tensor, coords: torch.Tensor, grad_out: torch.Tensor,
                  C: int, H: int, W: int, D: int, num_levels: int, radius: int, legacy: bool, dtype: int):
    """d loss / d fmap1 (B, C, Nq) and d loss / d fmap2 (B, C, H, W, D), both float32, from the gradient of
    a lookup output (B, L*(2r+1)^3, Nq) (dvc_corr_backward)."""
    _need_cuda(packed_q, packed_t, coords, grad_out)
    _expect_layout(packed_t, dtype, "corr_backward")
    B, Nq, _ = packed_q.shape
    c = _f32c(coords)
    g = _f32c(grad_out)
    dev = packed_q.device
    d1 = torch.empty((B, C, Nq), dtype=torch.float32, device=dev)
    d2 = torch.empty((B, C, H, W, D), dtype=torch.float32, device=dev)
    nws = lib().dvc_corr_backward_workspace_bytes_dtype(B, Nq, C, H, W, D, num_levels, radius, dtype)
    ws = torch.empty((max(nws, 256),), dtype=torch.uint8, device=dev)
    check(lib().dvc_corr_backward(_ptr(packed_q), _ptr(packed_t), _ptr(c), _ptr(g), _ptr(d1), _ptr(d2), _ptr(ws), B,
                                  Nq, C, H, W, D, num_levels, radius, DVC_LEGACY if legacy else DVC_FIXED, dtype,
                                  _stream(packed_q)), "corr_backward")
    return d1, d2


@_on_device
def sample3d(vol: torch.Tensor, pts: torch.Tensor, legacy: bool) -> torch.Tensor:
    _need_cuda(vol, pts)
    v = _f32c(vol)
    p = _f32c(pts)
    B, C, Hv, Wv, Dv = v.shape
    Nq = p.numel() // (3 * B)
    out = torch.empty((B, C, Nq), dtype=torch.float32, device=v.device)
    check(lib().dvc_sample3d(_ptr(v), _ptr(p), _ptr(out), B, C, Hv, Wv, Dv, Nq,
                             DVC_LEGACY if legacy else DVC_FIXED, _stream(v)), "sample3d")
    return out


def coords_grid(B: int, H: int, W: int, D: int, device) -> torch.Tensor:
    out = torch.empty((B, 3, H, W, D), dtype=torch.float32, device=device)
    _need_cuda(out)
    with torch.cuda.device(out.device):
        check(lib().dvc_coords_grid(_ptr(out), B, H, W, D, _stream(out)), "coords_grid")
    return out


@_on_device
def upflow(flow: torch.Tensor, target_shape) -> torch.Tensor:
    _need_cuda(flow)
    f = _f32c(flow)
    if f.dim() != 5:
        raise ValueError(f"upflow_3d expects (B, C, H, W, D), got {tuple(f.shape)}")
    B, C, h, w, d = f.shape
    H, W, D = (int(v) for v in target_shape)
    out = torch.empty((B, C, H, W, D), dtype=torch.float32, device=f.device)
    check(lib().dvc_upflow(_ptr(f), _ptr(out), B, C, h, w, d, H, W, D, _stream(f)), "upflow")
    return out


@_on_device
def flow_step(coords1: torch.Tensor, delta_flow, target_shape):
    """(coords1 + delta_flow, upflow_3d(coords1 + delta_flow - coords0, target_shape)) in one pass."""
    _need_cuda(coords1)
    c = _f32c(coords1)
    if c.dim() != 5 or c.shape[1] != 3:
        raise ValueError(f"coords1 must be (B, 3, H, W, D), got {tuple(c.shape)}")
    B, _, h, w, d = c.shape
    H, W, D = (int(v) for v in target_shape)
    dl = None
    if delta_flow is not None:
        _need_cuda(delta_flow)
        dl = _f32c(delta_flow)
        if dl.shape != c.shape:
            raise ValueError(f"delta_flow {tuple(dl.shape)} does not match coords1 {tuple(c.shape)}")
    new = torch.empty_like(c)
    up = torch.empty((B, 3, H, W, D), dtype=torch.float32, device=c.device)
    check(lib().dvc_flow_step(_ptr(c), None if dl is None else _ptr(dl), _ptr(new), _ptr(up), B, h, w, d, H, W, D,
                              _stream(c)), "flow_step")
    return new, up


def _nbytes(t: torch.Tensor) -> int:
    return t.numel() * t.element_size()


def _check_packed(what: str, packed: torch.Tensor, need: int, hint: str) -> None:
    """A packed-weights buffer has the byte count its kernel will read (need = 0: no kernel for these shapes)."""
    if need == 0 or _nbytes(packed) != need:
        raise ValueError(f"{what}: packed weights of {_nbytes(packed)} bytes; {hint}")


_GRU_AXES = ("h", "w", "d")


@_on_device
def gru_pack(weights, dtype: int) -> torch.Tensor:
    """The eighteen SepConvGRU3D tensors (state_dict names conv{z,r,q}_{h,w,d}.{weight,bias}) -> one buffer of the
    three axes' packed MFMA operands and biases (dvc_gru_pack; 3 x dvc_gru_packed_bytes)."""
    wz = weights["convz_h.weight"]
    _need_cuda(wz)
    hidden, cin = int(wz.shape[0]), int(wz.shape[1])
    nbytes = lib().dvc_gru_packed_bytes(hidden, cin - hidden, dtype)
    if nbytes == 0:
        raise NotImplementedError(f"gru_pack: hidden={hidden} input={cin - hidden} is outside the kernel's shapes "
                                  f"(hidden {_lib.GRU_HIDDEN}, input 1..{_lib.GRU_MAX_INPUT})")
    out = torch.empty((3, nbytes // 4), dtype=torch.float32, device=wz.device)
    for a, ax in enumerate(_GRU_AXES):
        ws = [_f32c(weights[f"conv{g}_{ax}.weight"].detach().reshape(hidden, cin, 5)) for g in "zrq"]
        bs = [_f32c(weights[f"conv{g}_{ax}.bias"].detach()) for g in "zrq"]
        check(lib().dvc_gru_pack(*map(_ptr, ws + bs), _ptr(out[a]), hidden, cin - hidden, dtype, _stream(wz)),
              "gru_pack")
    return out


@_on_device
def sep_gru_pass(h: torch.Tensor, x: torch.Tensor, packed_axis: torch.Tensor, out: torch.Tensor, axis: int,
                 dtype: int) -> torch.Tensor:
    """One axis pass (dvc_sep_gru_pass): h, x, out contiguous float32, out not overlapping h."""
    _need_cuda(h, x, packed_axis, out)
    B, hidden, H, W, D = h.shape
    check(lib().dvc_sep_gru_pass(_ptr(h), _ptr(x), _ptr(packed_axis), _ptr(out), B, hidden, x.shape[1], H, W, D, axis,
                                 dtype, _stream(h)), "sep_gru_pass")
    return out


@_on_device
def sep_gru(h: torch.Tensor, x: torch.Tensor, packed: torch.Tensor, dtype: int) -> torch.Tensor:
    """SepConvGRU3D.forward (update.py:178-199): the h, w and d passes, ping-ponged between two new buffers (the
    caller's h is only read)."""
    _need_cuda(h, x, packed)
    h, x = _f32c(h), _f32c(x)
    need = 3 * lib().dvc_gru_packed_bytes(h.shape[1], x.shape[1], dtype)
    _check_packed("sep_gru", packed, need, f"hidden {h.shape[1]}, input {x.shape[1]} and this precision take {need} "
                  "(gru_pack with the same dtype)")
    a, b = torch.empty_like(h), torch.empty_like(h)
    sep_gru_pass(h, x, packed[0], a, 0, dtype)
    sep_gru_pass(a, x, packed[1], b, 1, dtype)
    sep_gru_pass(b, x, packed[2], a, 2, dtype)
    return a


def _gru_tensors(what: str, hidden_like, x=None) -> tuple:
    """(B, hidden, H, W, D) of contiguous float32 (B, hidden, H, W, D) tensors of one volume (x: (B, input, ...))."""
    ts = list(hidden_like) + ([] if x is None else [x])
    _need_cuda(*ts)
    for t in ts:
        _conv_operand(t, f"{what}: tensors")
        if t.ndim != 5 or t.shape[0] != ts[0].shape[0] or t.shape[2:] != ts[0].shape[2:]:
            raise ValueError(f"{what}: tensors must be (B, C, H, W, D) of one batch and volume; got "
                             f"{[tuple(v.shape) for v in ts]}")
    for t in hidden_like:
        if t.shape[1] != ts[0].shape[1]:
            raise ValueError(f"{what}: hidden-state tensors differ in channels: {[tuple(v.shape) for v in hidden_like]}")
    return tuple(ts[0].shape)


@_on_device
def sep_gru_pass_save(h: torch.Tensor, x: torch.Tensor, packed_axis: torch.Tensor, out: torch.Tensor,
                      save: torch.Tensor, axis: int, dtype: int) -> torch.Tensor:
    """One axis pass that also stores z, r, q (after tanh) into save (3, B, hidden, H, W, D) (dvc_sep_gru_pass_save);
    all tensors contiguous float32, out and save overlapping nothing."""
    B, hidden, H, W, D = _gru_tensors("sep_gru_pass_save", (h, out), x)
    _need_cuda(packed_axis, save)
    _conv_operand(save, "sep_gru_pass_save: save")
    if tuple(save.shape) != (3,) + tuple(h.shape):
        raise ValueError(f"sep_gru_pass_save: save {tuple(save.shape)} is not (3,) + h's {tuple(h.shape)}")
    check(lib().dvc_sep_gru_pass_save(_ptr(h), _ptr(x), _ptr(packed_axis), _ptr(out), _ptr(save), B, hidden,
                                      x.shape[1], H, W, D, axis, dtype, _stream(h)), "sep_gru_pass_save")
    return out


@_on_device
def sep_gru_save(h: torch.Tensor, x: torch.Tensor, packed: torch.Tensor, dtype: int):
    """sep_gru for training (dvc_sep_gru_pass_save): (h_out, saved).  saved is (11, B, hidden, H, W, D) float32: z, r, q
    (after tanh) of the h pass, of the w pass and of the d pass, then the hidden states after the h and the w pass --
    11 x 96 x B H W D floats, 138 MB at 32^3.  h_out is bit-identical to sep_gru's."""
    _need_cuda(h, x, packed)
    h, x = _f32c(h), _f32c(x)
    need = 3 * lib().dvc_gru_packed_bytes(h.shape[1], x.shape[1], dtype)
    _check_packed("sep_gru_save", packed, need, f"hidden {h.shape[1]}, input {x.shape[1]} and this precision take "
                  f"{need} (gru_pack with the same dtype)")
    saved = torch.empty((11,) + tuple(h.shape), dtype=torch.float32, device=h.device)
    out = torch.empty_like(h)
    src = h
    for a, dst in enumerate((saved[9], saved[10], out)):
        src = sep_gru_pass_save(src, x, packed[a], dst, saved[3 * a:3 * a + 3], a, dtype)
    return out, saved


@_on_device
def gru_pack_dgrad(weights, dtype: int) -> torch.Tensor:
    """The nine SepConvGRU3D weights -> the three axes' packed input-gradient operands (dvc_gru_pack_dgrad;
    3 x dvc_gru_dgrad_packed_bytes): W'[ci][o][t'] = W[o][ci][4 - t'] of wq and of (wz; wr)."""
    wz = weights["convz_h.weight"]
    _need_cuda(wz)
    hidden, cin = int(wz.shape[0]), int(wz.shape[1])
    nbytes = lib().dvc_gru_dgrad_packed_bytes(hidden, cin - hidden, dtype)
    if nbytes == 0:
        raise NotImplementedError(f"gru_pack_dgrad: hidden={hidden} input={cin - hidden} is outside the kernel's shapes "
                                  f"(hidden {_lib.GRU_HIDDEN}, input 1..{_lib.GRU_MAX_INPUT})")
    out = torch.empty((3, nbytes // 4), dtype=torch.float32, device=wz.device)
    for a, ax in enumerate(_GRU_AXES):
        ws = [_f32c(weights[f"conv{g}_{ax}.weight"].detach().reshape(hidden, cin, 5)) for g in "zrq"]
        check(lib().dvc_gru_pack_dgrad(*map(_ptr, ws), _ptr(out[a]), hidden, cin - hidden, dtype, _stream(wz)),
              "gru_pack_dgrad")
    return out


def _prep_chunks(H: int, W: int, D: int) -> int:
    return -(-(H * W * D) // _lib.CONV3_PREP_CHUNK)


@_on_device
def gru_grad_prep(g: torch.Tensor, z: torch.Tensor, q: torch.Tensor, h: torch.Tensor):
    """(a_q, a_z, dh0, db_q, db_z) of one axis pass (dvc_gru_grad_prep): a_q = g z (1 - q^2), a_z = g (q - h) z (1 - z),
    dh0 = g (1 - z) and the bias gradients of the q and z gates, summed in a fixed order."""
    B, hidden, H, W, D = _gru_tensors("gru_grad_prep", (g, z, q, h))
    aq, az, dh = torch.empty_like(g), torch.empty_like(g), torch.empty_like(g)
    dbq, dbz = (torch.empty(hidden, dtype=torch.float32, device=g.device) for _ in range(2))
    partial = torch.empty(2 * hidden * B * _prep_chunks(H, W, D), dtype=torch.float32, device=g.device)
    check(lib().dvc_gru_grad_prep(*map(_ptr, (g, z, q, h, aq, az, dh, dbq, dbz, partial)), B, hidden, H, W, D,
                                  _stream(g)), "gru_grad_prep")
    return aq, az, dh, dbq, dbz


@_on_device
def sep_gru_dgrad(aq: torch.Tensor, az: torch.Tensor, h: torch.Tensor, r: torch.Tensor, packed_axis: torch.Tensor,
                  dh: torch.Tensor, dx, axis: int, dx_add: bool, dtype: int):
    """The input gradient of one axis pass (dvc_sep_gru_dgrad): returns (a_r, db_r); dh (gru_grad_prep's dh0) becomes
    dL/dh of the pass in place; dx (None: skipped) receives, or with dx_add accumulates, dL/dx of the pass."""
    B, hidden, H, W, D = _gru_tensors("sep_gru_dgrad", (aq, az, h, r, dh), dx)
    _need_cuda(packed_axis)
    inp = 1 if dx is None else int(dx.shape[1])   # without dx the kernel computes the hidden tiles only
    need = lib().dvc_gru_dgrad_packed_bytes(hidden, inp, dtype)
    _check_packed("sep_gru_dgrad", packed_axis, need, f"hidden {hidden} and this precision take {need} "
                  "(gru_pack_dgrad with the same dtype)")
    ar = torch.empty_like(aq)
    dbr = torch.empty(hidden, dtype=torch.float32, device=aq.device)
    partial = torch.empty(hidden * B * _prep_chunks(H, W, D), dtype=torch.float32, device=aq.device)
    check(lib().dvc_sep_gru_dgrad(_ptr(aq), _ptr(az), _ptr(h), _ptr(r), _ptr(packed_axis), _ptr(ar), _ptr(dh),
                                  None if dx is None else _ptr(dx), _ptr(dbr), _ptr(partial), B, hidden, inp, H, W, D,
                                  axis, int(bool(dx_add)), dtype, _stream(aq)), "sep_gru_dgrad")
    return ar, dbr


def gru_wgrad_slabs(inp: int, B: int, H: int, W: int, D: int, axis: int):
    """(K-blocks, K-blocks per slab, slabs) of dvc_gru_wgrad's split-K (include/dvccorr.h): a K-block is
    GRU_WGRAD_LINES lines x GRU_WGRAD_POS positions along the axis, positions fastest."""
    length = (H, W, D)[axis]
    nkb = -(-(B * H * W * D // length) // _lib.GRU_WGRAD_LINES) * -(-length // _lib.GRU_WGRAD_POS)
    want = min(nkb, -(-_lib.GRU_WGRAD_TARGET // (3 * -(-(_lib.GRU_HIDDEN + inp) // 16))))
    per = -(-nkb // want)
    return nkb, per, -(-nkb // per)


@_on_device
def gru_wgrad(h: torch.Tensor, x: torch.Tensor, r: torch.Tensor, az: torch.Tensor, ar: torch.Tensor,
              aq: torch.Tensor, axis: int, dtype: int) -> torch.Tensor:
    """(3, hidden, hidden + input, 5) float32: the weight gradients of the z, r and q convolutions of one axis pass
    (dvc_gru_wgrad) from the pass's input h, x, its reset gate r and the gate gradients a_z, a_r, a_q."""
    B, hidden, H, W, D = _gru_tensors("gru_wgrad", (h, r, az, ar, aq), x)
    inp = int(x.shape[1])
    nws = lib().dvc_gru_wgrad_workspace_bytes(hidden, inp, B, H, W, D, axis)
    if nws == 0:
        raise NotImplementedError(f"gru_wgrad: hidden={hidden} input={inp} is outside the kernel's shapes "
                                  f"(hidden {_lib.GRU_HIDDEN}, input 1..{_lib.GRU_MAX_INPUT})")
    dw = torch.empty((3, hidden, hidden + inp, 5), dtype=torch.float32, device=h.device)
    ws = torch.empty(nws // 4, dtype=torch.float32, device=h.device)
    check(lib().dvc_gru_wgrad(*map(_ptr, (h, x, r, az, ar, aq, dw, ws)), B, hidden, inp, H, W, D, axis, dtype,
                              _stream(h)), "gru_wgrad")
    return dw


def _conv_operand(t: torch.Tensor, what: str) -> None:
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous float32, got {t.dtype} with strides {tuple(t.stride())}")


@_on_device
def conv3_pack(weight: torch.Tensor, bias: torch.Tensor, dtype: int) -> torch.Tensor:
    """A (cout, cin, 3, 3, 3) weight and its (cout) bias -> the packed MFMA operands and biases of dvc_conv3
    (dvc_conv3_pack; dvc_conv3_packed_bytes)."""
    _need_cuda(weight, bias)
    if weight.ndim != 5 or tuple(weight.shape[2:]) != (3, 3, 3) or tuple(bias.shape) != (weight.shape[0],):
        raise ValueError(f"conv3_pack: weight {tuple(weight.shape)} bias {tuple(bias.shape)} are not a 3 x 3 x 3 "
                         "convolution's")
    cout, cin = int(weight.shape[0]), int(weight.shape[1])
    nbytes = lib().dvc_conv3_packed_bytes(cin, cout, dtype)
    if nbytes == 0:
        raise NotImplementedError(f"conv3_pack: cin={cin} cout={cout} is outside the kernel's shapes "
                                  f"(cin 1..{_lib.CONV3_MAX_CIN}, cout 1..{_lib.CONV3_MAX_COUT})")
    w, b = _f32c(weight.detach()), _f32c(bias.detach())
    out = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
    check(lib().dvc_conv3_pack(_ptr(w), _ptr(b), _ptr(out), cin, cout, dtype, _stream(w)), "conv3_pack")
    return out


@_on_device
def conv3(src0: torch.Tensor, src1, packed: torch.Tensor, dst: torch.Tensor, dst_offset: int, cout: int, relu: bool,
          dtype: int) -> torch.Tensor:
    """dst[:, dst_offset:dst_offset + cout] = conv3x3x3(cat[src0, src1]) + bias (+ ReLU) (dvc_conv3); src1 may be
    None.  All tensors contiguous float32 (B, C, H, W, D); dst is written in place and returned."""
    ts = [src0, dst] + ([] if src1 is None else [src1])
    _need_cuda(packed, *ts)
    for t in ts:
        _conv_operand(t, "conv3: sources and dst")
        if t.ndim != 5 or t.shape[0] != src0.shape[0] or t.shape[2:] != src0.shape[2:]:
            raise ValueError(f"conv3: sources and dst must be (B, C, H, W, D) of one batch and volume; got "
                             f"{[tuple(v.shape) for v in ts]}")
    B, c0, H, W, D = src0.shape
    c1 = 0 if src1 is None else int(src1.shape[1])
    need = lib().dvc_conv3_packed_bytes(c0 + c1, cout, dtype)
    _check_packed("conv3", packed, need, f"cin {c0 + c1}, cout {cout} and this precision take {need} "
                  "(conv3_pack with the same dtype)")
    check(lib().dvc_conv3(_ptr(src0), c0, None if src1 is None else _ptr(src1), c1, _ptr(packed), _ptr(dst),
                          int(dst.shape[1]), int(dst_offset), int(cout), int(bool(relu)), B, H, W, D, dtype,
                          _stream(src0)), "conv3")
    return dst


@_on_device
def conv3_pack_dgrad(weight: torch.Tensor, dtype: int) -> torch.Tensor:
    """A (cout, cin, 3, 3, 3) weight -> the packed operands of its input gradient (dvc_conv3_pack_dgrad): the layer
    W'[ci][o][t'] = W[o][ci][26 - t'] with zero biases, so conv3(g, None, packed, dx, 0, cin, False, dtype) is
    d loss / d cat[x, x2]."""
    _need_cuda(weight)
    if weight.ndim != 5 or tuple(weight.shape[2:]) != (3, 3, 3):
        raise ValueError(f"conv3_pack_dgrad: weight {tuple(weight.shape)} is not a 3 x 3 x 3 convolution's")
    cout, cin = int(weight.shape[0]), int(weight.shape[1])
    nbytes = lib().dvc_conv3_packed_bytes(cout, cin, dtype)
    if nbytes == 0:
        raise NotImplementedError(f"conv3_pack_dgrad: cin={cin} cout={cout} is outside the kernel's shapes "
                                  f"(cin 1..{_lib.CONV3_MAX_CIN}, cout 1..{_lib.CONV3_MAX_COUT})")
    w = _f32c(weight.detach())
    out = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
    check(lib().dvc_conv3_pack_dgrad(_ptr(w), _ptr(out), cin, cout, dtype, _stream(w)), "conv3_pack_dgrad")
    return out


@_on_device
def conv3_grad_prep(grad_y: torch.Tensor, y, relu: bool):
    """(g, db) of a layer's output gradient (dvc_conv3_grad_prep): g = grad_y * (y > 0) with ReLU (y the layer's own
    output), else grad_y itself (no copy); db[o] = sum over (b, v) of g[b, o, v], summed in a fixed order."""
    _need_cuda(grad_y)
    _conv_operand(grad_y, "conv3_grad_prep: grad_y")
    if grad_y.ndim != 5:
        raise ValueError(f"conv3_grad_prep: grad_y must be (B, C, H, W, D), got {tuple(grad_y.shape)}")
    g = None
    if relu:
        _need_cuda(y)
        _conv_operand(y, "conv3_grad_prep: y")
        if y.shape != grad_y.shape:
            raise ValueError(f"conv3_grad_prep: y {tuple(y.shape)} does not match grad_y {tuple(grad_y.shape)}")
        g = torch.empty_like(grad_y)
    B, cout, H, W, D = grad_y.shape
    nchunk = -(-(H * W * D) // _lib.CONV3_PREP_CHUNK)
    db = torch.empty(cout, dtype=torch.float32, device=grad_y.device)
    partial = torch.empty(cout * B * nchunk, dtype=torch.float32, device=grad_y.device)
    check(lib().dvc_conv3_grad_prep(_ptr(grad_y), _ptr(y) if relu else None, _ptr(g) if relu else None, _ptr(db),
                                    _ptr(partial), cout, B, H, W, D, _stream(grad_y)), "conv3_grad_prep")
    return (g if relu else grad_y), db


def conv3_wgrad_slabs(cin: int, cout: int, B: int, H: int, W: int, D: int):
    """(K-blocks, K-blocks per slab, slabs) of dvc_conv3_wgrad's split-K (include/dvccorr.h): the K-blocks are the
    CONV3_WGRAD_KH x KW x KD voxel boxes of the (B, H, W, D) grid in that order, D fastest."""
    nbox = B * -(-H // _lib.CONV3_WGRAD_KH) * -(-W // _lib.CONV3_WGRAD_KW) * -(-D // _lib.CONV3_WGRAD_KD)
    groups = 1 if cout <= 16 else -(-cout // 32)
    want = min(nbox, -(-_lib.CONV3_WGRAD_TARGET // (-(-cin // 16) * groups)))
    per = -(-nbox // want)
    return nbox, per, -(-nbox // per)


@_on_device
def conv3_wgrad(x: torch.Tensor, x2, g: torch.Tensor, dtype: int) -> torch.Tensor:
    """dW (cout, cin, 3, 3, 3) float32 of a 3 x 3 x 3 layer from its input cat[x, x2] (x2 may be None) and its masked
    output gradient g (dvc_conv3_wgrad).  All tensors contiguous float32 (B, C, H, W, D)."""
    ts = [x, g] + ([] if x2 is None else [x2])
    _need_cuda(*ts)
    for t in ts:
        _conv_operand(t, "conv3_wgrad: x, x2 and g")
        if t.ndim != 5 or t.shape[0] != x.shape[0] or t.shape[2:] != x.shape[2:]:
            raise ValueError(f"conv3_wgrad: x, x2 and g must be (B, C, H, W, D) of one batch and volume; got "
                             f"{[tuple(v.shape) for v in ts]}")
    B, c0, H, W, D = x.shape
    c1 = 0 if x2 is None else int(x2.shape[1])
    cout = int(g.shape[1])
    nws = lib().dvc_conv3_wgrad_workspace_bytes(c0 + c1, cout, B, H, W, D)
    if nws == 0:
        raise NotImplementedError(f"conv3_wgrad: cin={c0 + c1} cout={cout} is outside the kernel's shapes "
                                  f"(cin 1..{_lib.CONV3_MAX_CIN}, cout 1..{_lib.CONV3_MAX_COUT})")
    dw = torch.empty((cout, c0 + c1, 3, 3, 3), dtype=torch.float32, device=x.device)
    ws = torch.empty(nws // 4, dtype=torch.float32, device=x.device)
    check(lib().dvc_conv3_wgrad(_ptr(x), c0, None if x2 is None else _ptr(x2), c1, _ptr(g), cout, _ptr(dw), _ptr(ws),
                                B, H, W, D, dtype, _stream(x)), "conv3_wgrad")
    return dw


@_on_device
def conv7_flow_pack(weight: torch.Tensor, bias: torch.Tensor, dtype: int) -> torch.Tensor:
    """encoder.convf1's (64, 3, 7, 7, 7) weight and (64) bias -> the packed operands of dvc_conv7_flow."""
    _need_cuda(weight, bias)
    if tuple(weight.shape) != (_lib.CONV7_COUT, 3, 7, 7, 7) or tuple(bias.shape) != (_lib.CONV7_COUT,):
        raise NotImplementedError(f"conv7_flow_pack: weight {tuple(weight.shape)} bias {tuple(bias.shape)}; the "
                                  f"kernel covers ({_lib.CONV7_COUT}, 3, 7, 7, 7)")
    nbytes = lib().dvc_conv7_flow_packed_bytes(dtype)
    if nbytes == 0:
        raise ValueError(f"conv7_flow_pack: bad dtype {dtype}")
    w, b = _f32c(weight.detach()), _f32c(bias.detach())
    out = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
    check(lib().dvc_conv7_flow_pack(_ptr(w), _ptr(b), _ptr(out), dtype, _stream(w)), "conv7_flow_pack")
    return out


@_on_device
def conv7_flow(flow: torch.Tensor, packed: torch.Tensor, dst: torch.Tensor, dtype: int) -> torch.Tensor:
    """dst = relu(convf1(flow)): flow (B, 3, H, W, D), dst (B, 64, H, W, D), contiguous float32 (dvc_conv7_flow);
    dst is written in place and returned."""
    _need_cuda(flow, packed, dst)
    _conv_operand(flow, "conv7_flow: flow")
    _conv_operand(dst, "conv7_flow: dst")
    if flow.ndim != 5 or dst.ndim != 5 or flow.shape[1] != 3 or dst.shape[1] != _lib.CONV7_COUT \
            or dst.shape[0] != flow.shape[0] or dst.shape[2:] != flow.shape[2:]:
        raise ValueError(f"conv7_flow: flow must be (B, 3, H, W, D) and dst (B, {_lib.CONV7_COUT}, H, W, D); got "
                         f"{tuple(flow.shape)} and {tuple(dst.shape)}")
    need = lib().dvc_conv7_flow_packed_bytes(dtype)
    _check_packed("conv7_flow", packed, need, f"this precision takes {need} (conv7_flow_pack with the same dtype)")
    B, _, H, W, D = flow.shape
    check(lib().dvc_conv7_flow(_ptr(flow), _ptr(packed), _ptr(dst), B, H, W, D, dtype, _stream(flow)), "conv7_flow")
    return dst


def conv7_wgrad_slabs(B: int, H: int, W: int, D: int):
    """(K-blocks, K-blocks per slab, slabs) of dvc_conv7_wgrad's split-K (include/dvccorr.h): the K-blocks are the
    CONV7_WGRAD_KH x KW x KD voxel boxes of the (B, H, W, D) grid in that order, D fastest."""
    nbox = B * -(-H // _lib.CONV7_WGRAD_KH) * -(-W // _lib.CONV7_WGRAD_KW) * -(-D // _lib.CONV7_WGRAD_KD)
    groups = -(-(-(-3 * 343 // 16)) // _lib.CONV7_WGRAD_TILES)
    want = min(nbox, -(-_lib.CONV7_WGRAD_TARGET // groups))
    per = -(-nbox // want)
    return nbox, per, -(-nbox // per)


@_on_device
def conv7_wgrad(flow: torch.Tensor, g: torch.Tensor, dtype: int) -> torch.Tensor:
    """dW (64, 3, 7, 7, 7) float32 of encoder.convf1 from its input flow (B, 3, H, W, D) and its masked output
    gradient g (B, 64, H, W, D), both contiguous float32 (dvc_conv7_wgrad)."""
    _need_cuda(flow, g)
    _conv_operand(flow, "conv7_wgrad: flow")
    _conv_operand(g, "conv7_wgrad: g")
    if flow.ndim != 5 or g.ndim != 5 or flow.shape[1] != 3 or g.shape[1] != _lib.CONV7_COUT \
            or g.shape[0] != flow.shape[0] or g.shape[2:] != flow.shape[2:]:
        raise ValueError(f"conv7_wgrad: flow must be (B, 3, H, W, D) and g (B, {_lib.CONV7_COUT}, H, W, D); got "
                         f"{tuple(flow.shape)} and {tuple(g.shape)}")
    B, _, H, W, D = flow.shape
    nws = lib().dvc_conv7_wgrad_workspace_bytes(B, H, W, D)
    if nws == 0:
        raise NotImplementedError(f"conv7_wgrad: B={B} volume {(H, W, D)} is outside the kernel's shapes")
    dw = torch.empty((_lib.CONV7_COUT, 3, 7, 7, 7), dtype=torch.float32, device=flow.device)
    ws = torch.empty(nws // 4, dtype=torch.float32, device=flow.device)
    check(lib().dvc_conv7_wgrad(_ptr(flow), _ptr(g), _ptr(dw), _ptr(ws), B, H, W, D, dtype, _stream(flow)),
          "conv7_wgrad")
    return dw


__all__ = ["pack_queries", "pack_targets", "pack_targets_gathered", "build", "pool", "lookup", "lookup_fused", "lookup_fused_proj", "corr_backward", "sample3d",
           "proj_pack", "proj_pack_cached", "lookup_proj",
           "coords_grid", "upflow", "flow_step",
           "fused_workspace", "dtype_code", "layout", "bricked_levels", "DVC_BRICKED", "_lib"]


# ---------------------------------------------------------------------------------------------------------------
# the encoders' forward (csrc/encoder.hip)
# ---------------------------------------------------------------------------------------------------------------
def enc_out_extent(n: int, stride: int) -> int:
    """Output extent of a 7^3 / padding 3, 3^3 / padding 1 or 1^3 / padding 0 convolution with this stride."""
    return (int(n) - 1) // int(stride) + 1


def enc_out_volume(vol, stride: int):
    return tuple(enc_out_extent(n, stride) for n in vol)


def enc_covers(taps: int, cin: int, cout: int) -> bool:
    """Channel counts k_enc_conv runs (dvc_enc_conv)."""
    return taps in (1, 27) and cin % 8 == 0 and 8 <= cin <= _lib.ENC_MAX_CIN and 1 <= cout <= _lib.ENC_MAX_COUT


def enc_partials(taps: int, stride: int, cout: int, B: int, ovol, device) -> torch.Tensor:
    """The statistics partials buffer of one layer's output (dvc_enc_partials_bytes), as float64."""
    n = lib().dvc_enc_partials_bytes(taps, stride, cout, B, *ovol)
    if n == 0:
        raise ValueError(f"enc_partials: taps={taps} stride={stride} cout={cout} B={B} volume {tuple(ovol)}")
    return torch.empty(n // 8, dtype=torch.float64, device=device)


@_on_device
def enc_stem_pack(weight: torch.Tensor, bias: torch.Tensor, dtype: int) -> torch.Tensor:
    """conv1's (32, 1, 7, 7, 7) weight and (32) bias -> the packed operands of dvc_enc_stem."""
    _need_cuda(weight, bias)
    if tuple(weight.shape) != (_lib.ENC_STEM_COUT, 1, 7, 7, 7) or tuple(bias.shape) != (_lib.ENC_STEM_COUT,):
        raise NotImplementedError(f"enc_stem_pack: weight {tuple(weight.shape)} bias {tuple(bias.shape)}; the kernel "
                                  f"covers ({_lib.ENC_STEM_COUT}, 1, 7, 7, 7)")
    nbytes = lib().dvc_enc_stem_packed_bytes(dtype)
    if nbytes == 0:
        raise ValueError(f"enc_stem_pack: bad dtype {dtype}")
    w, b = _f32c(weight.detach()), _f32c(bias.detach())
    out = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
    check(lib().dvc_enc_stem_pack(_ptr(w), _ptr(b), _ptr(out), dtype, _stream(w)), "enc_stem_pack")
    return out


def _enc_partials_ok(what, partials, taps, stride, cout, B, ovol) -> None:
    if partials is None:
        return
    need = lib().dvc_enc_partials_bytes(taps, stride, cout, B, *ovol)
    if partials.dtype != torch.float64 or not partials.is_contiguous() or _nbytes(partials) != need or need == 0:
        raise ValueError(f"{what}: partials must be contiguous float64 of {need} bytes (enc_partials), got "
                         f"{partials.dtype} of {_nbytes(partials)}")


@_on_device
def enc_stem(x: torch.Tensor, packed: torch.Tensor, y: torch.Tensor, partials, stride: int, dtype: int) -> torch.Tensor:
    """y = conv1(x) + bias, raw: x (B, 1, H, W, D), y (B, 32, OH, OW, OD), contiguous float32 (dvc_enc_stem);
    `partials` (enc_partials with taps = 343), where given, receives the statistics partials of y."""
    _need_cuda(x, packed, y)
    _conv_operand(x, "enc_stem: x")
    _conv_operand(y, "enc_stem: y")
    if stride not in (1, 2):
        raise ValueError(f"enc_stem: stride {stride} is not 1 or 2")
    if x.ndim != 5 or x.shape[1] != 1 or y.ndim != 5 or \
            tuple(y.shape) != (x.shape[0], _lib.ENC_STEM_COUT) + enc_out_volume(x.shape[2:], stride):
        raise ValueError(f"enc_stem: x must be (B, 1, H, W, D) and y (B, {_lib.ENC_STEM_COUT}, OH, OW, OD) of stride "
                         f"{stride}; got {tuple(x.shape)} and {tuple(y.shape)}")
    need = lib().dvc_enc_stem_packed_bytes(dtype)
    _check_packed("enc_stem", packed, need, f"this precision takes {need} (enc_stem_pack with the same dtype)")
    B, _, H, W, D = x.shape
    _enc_partials_ok("enc_stem", partials, _lib.ENC_STEM_TAPS, stride, _lib.ENC_STEM_COUT, B, y.shape[2:])
    check(lib().dvc_enc_stem(_ptr(x), _ptr(packed), _ptr(y), None if partials is None else _ptr(partials), B, H, W, D,
                             stride, dtype, _stream(x)), "enc_stem")
    return y


@_on_device
def enc_conv_pack(weight: torch.Tensor, bias: torch.Tensor, dtype: int) -> torch.Tensor:
    """A (cout, cin, 3, 3, 3) or (cout, cin, 1, 1, 1) weight and its bias -> the packed operands of dvc_enc_conv."""
    _need_cuda(weight, bias)
    if weight.ndim != 5 or tuple(weight.shape[2:]) not in ((3, 3, 3), (1, 1, 1)) or \
            tuple(bias.shape) != (weight.shape[0],):
        raise ValueError(f"enc_conv_pack: weight {tuple(weight.shape)} bias {tuple(bias.shape)} are not a 3 x 3 x 3 or "
                         "1 x 1 x 1 convolution's")
    cout, cin, taps = int(weight.shape[0]), int(weight.shape[1]), int(weight.shape[2]) ** 3
    nbytes = lib().dvc_enc_conv_packed_bytes(taps, cin, cout, dtype)
    if nbytes == 0:
        raise NotImplementedError(f"enc_conv_pack: cin={cin} cout={cout} is outside the kernel's shapes (cin a "
                                  f"multiple of 8 up to {_lib.ENC_MAX_CIN}, cout 1..{_lib.ENC_MAX_COUT})")
    w, b = _f32c(weight.detach()), _f32c(bias.detach())
    out = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
    check(lib().dvc_enc_conv_pack(_ptr(w), _ptr(b), _ptr(out), taps, cin, cout, dtype, _stream(w)), "enc_conv_pack")
    return out


@_on_device
def enc_conv(x: torch.Tensor, scale_shift, prologue: int, packed: torch.Tensor, y: torch.Tensor, y2, partials,
             taps: int, stride: int, dtype: int) -> torch.Tensor:
    """y = conv(prologue(x)) + bias (dvc_enc_conv): taps 27 (3 x 3 x 3, padding 1) or 1, stride 1 or 2; prologue 0
    identity, 1 ReLU, 2 relu(x scale + shift) with scale_shift (B, cin, 2).  With y2 the output is split (the
    context encoder's conv2): y gets tanh of the first y.shape[1] channels, y2 the ReLU of the rest.  `partials`
    (enc_partials), where given, receives the statistics partials of the raw output."""
    ts = [x, y] + ([] if y2 is None else [y2]) + ([] if scale_shift is None else [scale_shift])
    _need_cuda(packed, *ts)
    for t in ts:
        _conv_operand(t, "enc_conv: x, scale_shift, y and y2")
    if taps not in (1, 27) or stride not in (1, 2) or prologue not in (0, 1, 2):
        raise ValueError(f"enc_conv: taps {taps} (1 or 27), stride {stride} (1 or 2), prologue {prologue} (0, 1 or 2)")
    if x.ndim != 5:
        raise ValueError(f"enc_conv: x must be (B, C, H, W, D), got {tuple(x.shape)}")
    B, cin, H, W, D = x.shape
    ovol = enc_out_volume((H, W, D), stride)
    for t in [y] + ([] if y2 is None else [y2]):
        if t.ndim != 5 or t.shape[0] != B or tuple(t.shape[2:]) != ovol:
            raise ValueError(f"enc_conv: an output of x {tuple(x.shape)} at stride {stride} must be (B, C) + {ovol}; "
                             f"got {tuple(t.shape)}")
    cout = int(y.shape[1]) + (0 if y2 is None else int(y2.shape[1]))
    split = -1 if y2 is None else int(y.shape[1])
    if scale_shift is not None and tuple(scale_shift.shape) != (B, cin, 2):
        raise ValueError(f"enc_conv: scale_shift must be {(B, cin, 2)}, got {tuple(scale_shift.shape)}")
    if prologue == 2 and scale_shift is None:
        raise ValueError("enc_conv: prologue 2 needs scale_shift")
    need = lib().dvc_enc_conv_packed_bytes(taps, cin, cout, dtype)
    _check_packed("enc_conv", packed, need, f"taps {taps}, cin {cin}, cout {cout} and this precision take {need} "
                  "(enc_conv_pack with the same dtype)")
    _enc_partials_ok("enc_conv", partials, taps, stride, cout, B, ovol)
    check(lib().dvc_enc_conv(_ptr(x), None if scale_shift is None else _ptr(scale_shift), prologue, _ptr(packed),
                             _ptr(y), None if y2 is None else _ptr(y2), split,
                             None if partials is None else _ptr(partials), taps, stride, cin, cout, B, H, W, D, dtype,
                             _stream(x)), "enc_conv")
    return y


@_on_device
def enc_stats(partials: torch.Tensor, scale_shift: torch.Tensor, taps: int, stride: int, ovol, eps: float) -> torch.Tensor:
    """scale_shift (B, C, 2) <- (1 / sqrt(var + eps), -mean scale) per (b, c) from the partials of a layer's output
    of volume ovol (dvc_enc_stats); taps and stride are the producing layer's (taps = 343: the stem)."""
    _need_cuda(partials, scale_shift)
    _conv_operand(scale_shift, "enc_stats: scale_shift")
    if scale_shift.ndim != 3 or scale_shift.shape[2] != 2:
        raise ValueError(f"enc_stats: scale_shift must be (B, C, 2), got {tuple(scale_shift.shape)}")
    B, C, _ = scale_shift.shape
    if partials is None:
        raise ValueError("enc_stats: partials is None")
    _enc_partials_ok("enc_stats", partials, taps, stride, C, B, ovol)
    check(lib().dvc_enc_stats(_ptr(partials), _ptr(scale_shift), taps, stride, C, B, *[int(v) for v in ovol],
                              float(eps), _stream(partials)), "enc_stats")
    return scale_shift


@_on_device
def enc_residual(c3: torch.Tensor, ss3, shortcut: torch.Tensor, ss4, mode: int, out: torch.Tensor) -> torch.Tensor:
    """out = relu(c3 scale3 + shift3 + r), r = shortcut (mode 0), shortcut scale4 + shift4 (1) or its ReLU (2); a
    None table is scale 1, shift 0 (dvc_enc_residual).  All (B, C, H, W, D) contiguous float32."""
    ts = [c3, shortcut, out] + [t for t in (ss3, ss4) if t is not None]
    _need_cuda(*ts)
    for t in ts:
        _conv_operand(t, "enc_residual: tensors")
    if c3.ndim != 5 or shortcut.shape != c3.shape or out.shape != c3.shape:
        raise ValueError(f"enc_residual: c3, shortcut and out must be one (B, C, H, W, D) shape; got "
                         f"{tuple(c3.shape)}, {tuple(shortcut.shape)}, {tuple(out.shape)}")
    B, C, H, W, D = c3.shape
    for t in (ss3, ss4):
        if t is not None and tuple(t.shape) != (B, C, 2):
            raise ValueError(f"enc_residual: a scale_shift table must be {(B, C, 2)}, got {tuple(t.shape)}")
    if mode not in (0, 1, 2):
        raise ValueError(f"enc_residual: mode {mode} is not 0, 1 or 2")
    check(lib().dvc_enc_residual(_ptr(c3), None if ss3 is None else _ptr(ss3), _ptr(shortcut),
                                 None if ss4 is None else _ptr(ss4), mode, _ptr(out), C, B, H, W, D, _stream(c3)),
          "enc_residual")
    return out


# ---------------------------------------------------------------------------------------------------------------
# the encoders' backward (csrc/encoder_grad.hip)
# ---------------------------------------------------------------------------------------------------------------
def enc_grad_covers(taps: int, cin: int, cout: int) -> bool:
    """Channel counts the backward kernels of an encoder convolution run (dvc_enc_wgrad, dvc_enc_dgrad)."""
    return (taps in (1, 27) and cin % 8 == 0 and 8 <= cin <= _lib.ENC_MAX_COUT and 1 <= cout <= _lib.ENC_MAX_COUT
            and cout % 8 == 0)


def enc_wgrad_slabs(taps: int, stride: int, cin: int, cout: int, B: int, vol):
    """(K steps, K steps per slab, slabs) of dvc_enc_wgrad's split-K (include/dvccorr.h)."""
    ohwd = 1
    for n in enc_out_volume(vol, stride):
        ohwd *= n
    nk = B * -(-ohwd // 32)
    groups = -(-(-(-taps * cin // 16)) // (2 if taps == 1 else 7)) * -(-cout // 32)
    want = min(-(-nk // 4), -(-_lib.ENC_WGRAD_TARGET // groups))
    per = -(-nk // want)
    return nk, per, -(-nk // per)


def _enc_5d(what, *ts):
    _need_cuda(*ts)
    for t in ts:
        _conv_operand(t, what)
        if t.ndim != 5:
            raise ValueError(f"{what} must be (B, C, H, W, D), got {tuple(t.shape)}")


@_on_device
def enc_norm_grad(g: torch.Tensor, x, scale_shift, mask: bool, want_gx: bool = True, want_db: bool = True):
    """(g_x | None, db | None) of a raw convolution output x (B, C, H, W, D) from the gradient g with respect to its
    normalised value (dvc_enc_norm_grad): gn = g [fma(x, scale, shift) > 0] under `mask`, g_x = scale (gn - mean(gn) -
    n mean(gn n)); scale_shift None: g_x = gn with the mask [x > 0]."""
    ts = [g] + ([x] if x is not None else [])
    _enc_5d("enc_norm_grad: g and x", *ts)
    if x is not None and x.shape != g.shape:
        raise ValueError(f"enc_norm_grad: g {tuple(g.shape)} and x {tuple(x.shape)} differ")
    if x is None and (mask or scale_shift is not None):
        raise ValueError("enc_norm_grad: a mask or a table needs x")
    B, C, H, W, D = g.shape
    if scale_shift is not None:
        _need_cuda(scale_shift)
        _conv_operand(scale_shift, "enc_norm_grad: scale_shift")
        if tuple(scale_shift.shape) != (B, C, 2):
            raise ValueError(f"enc_norm_grad: scale_shift must be {(B, C, 2)}, got {tuple(scale_shift.shape)}")
    if not (want_gx or want_db):
        raise ValueError("enc_norm_grad: neither g_x nor db asked for")
    nbytes = lib().dvc_enc_grad_partials_bytes(C, B, H, W, D)
    if nbytes == 0:
        raise ValueError(f"enc_norm_grad: bad shape {tuple(g.shape)}")
    part = torch.empty(nbytes // 8, dtype=torch.float64, device=g.device)
    gx = torch.empty_like(g) if want_gx else None
    db = torch.empty(C, dtype=torch.float32, device=g.device) if want_db else None
    check(lib().dvc_enc_norm_grad(_ptr(g), None if x is None else _ptr(x), None if scale_shift is None else
                                  _ptr(scale_shift), 1 if mask else 0, None if gx is None else _ptr(gx),
                                  None if db is None else _ptr(db), _ptr(part), C, B, H, W, D, _stream(g)),
          "enc_norm_grad")
    return gx, db


@_on_device
def enc_grad_add(a: torch.Tensor, b, m) -> torch.Tensor:
    """(a + b) [m > 0], b and m optional, same shapes, contiguous float32 (dvc_enc_grad_add)."""
    ts = [t for t in (a, b, m) if t is not None]
    _need_cuda(*ts)
    for t in ts:
        _conv_operand(t, "enc_grad_add: tensors")
        if t.shape != a.shape:
            raise ValueError(f"enc_grad_add: shapes differ: {[tuple(v.shape) for v in ts]}")
    dst = torch.empty_like(a)
    check(lib().dvc_enc_grad_add(_ptr(a), None if b is None else _ptr(b), None if m is None else _ptr(m), _ptr(dst),
                                 a.numel(), _stream(a)), "enc_grad_add")
    return dst


@_on_device
def enc_split_grad(g_net, g_ctx, net: torch.Tensor, ctx: torch.Tensor) -> torch.Tensor:
    """The gradient of the context encoder's conv2 output (B, hidden + context, ..) from the gradients of its tanh and
    ReLU halves (either may be None: zero) and the stored halves (dvc_enc_split_grad)."""
    ts = [t for t in (g_net, g_ctx, net, ctx) if t is not None]
    _enc_5d("enc_split_grad: tensors", *ts)
    if (g_net is not None and g_net.shape != net.shape) or (g_ctx is not None and g_ctx.shape != ctx.shape) or \
            net.shape[0] != ctx.shape[0] or net.shape[2:] != ctx.shape[2:]:
        raise ValueError(f"enc_split_grad: shapes {[tuple(v.shape) for v in ts]}")
    B, split, H, W, D = net.shape
    cout = split + int(ctx.shape[1])
    g = torch.empty((B, cout, H, W, D), dtype=torch.float32, device=net.device)
    check(lib().dvc_enc_split_grad(None if g_net is None else _ptr(g_net), None if g_ctx is None else _ptr(g_ctx),
                                   _ptr(net), _ptr(ctx), _ptr(g), split, cout, B, H, W, D, _stream(net)),
          "enc_split_grad")
    return g


def _enc_taps(weight, what):
    if weight.ndim != 5 or tuple(weight.shape[2:]) not in ((3, 3, 3), (1, 1, 1)):
        raise ValueError(f"{what}: weight {tuple(weight.shape)} is not a 3 x 3 x 3 or 1 x 1 x 1 convolution's")
    return 27 if weight.shape[2] == 3 else 1


@_on_device
def enc_conv_pack_dgrad(weight: torch.Tensor, dtype: int) -> torch.Tensor:
    """A (cout, cin, 3, 3, 3) or (cout, cin, 1, 1, 1) weight -> the packed operands of its input gradient
    (dvc_enc_conv_pack_dgrad): transposed, flipped, zero biases."""
    _need_cuda(weight)
    taps = _enc_taps(weight, "enc_conv_pack_dgrad")
    cout, cin = int(weight.shape[0]), int(weight.shape[1])
    nbytes = lib().dvc_enc_dgrad_packed_bytes(taps, cin, cout, dtype)
    if nbytes == 0:
        raise NotImplementedError(f"enc_conv_pack_dgrad: cin={cin} cout={cout} taps={taps} is outside the kernel's shapes")
    w = _f32c(weight.detach())
    out = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
    check(lib().dvc_enc_conv_pack_dgrad(_ptr(w), _ptr(out), taps, cin, cout, dtype, _stream(w)), "enc_conv_pack_dgrad")
    return out


@_on_device
def enc_dgrad(g: torch.Tensor, packed: torch.Tensor, taps: int, stride: int, cin: int, vol, dtype: int) -> torch.Tensor:
    """dx (B, cin) + vol of a layer with input volume `vol` from its output gradient g (B, cout, OH, OW, OD)
    (dvc_enc_dgrad); packed from enc_conv_pack_dgrad with the same dtype."""
    _enc_5d("enc_dgrad: g", g)
    _need_cuda(packed)
    vol = tuple(int(v) for v in vol)
    if taps not in (1, 27) or stride not in (1, 2) or len(vol) != 3 or tuple(g.shape[2:]) != enc_out_volume(vol, stride):
        raise ValueError(f"enc_dgrad: taps {taps}, stride {stride}, g {tuple(g.shape)} for an input volume {vol}")
    B, cout = int(g.shape[0]), int(g.shape[1])
    need = lib().dvc_enc_dgrad_packed_bytes(taps, cin, cout, dtype)
    _check_packed("enc_dgrad", packed, need, f"taps {taps}, cin {cin}, cout {cout} and this precision take {need} "
                  "(enc_conv_pack_dgrad with the same dtype)")
    dx = torch.empty((B, cin) + vol, dtype=torch.float32, device=g.device)
    check(lib().dvc_enc_dgrad(_ptr(g), _ptr(packed), _ptr(dx), taps, stride, cin, cout, B, *vol, dtype, _stream(g)),
          "enc_dgrad")
    return dx


@_on_device
def enc_wgrad(x: torch.Tensor, scale_shift, prologue: int, g: torch.Tensor, taps: int, stride: int, dtype: int) -> torch.Tensor:
    """dW (cout, cin, k, k, k) float32 of an encoder convolution from its raw input x, the prologue the forward applied
    to it and the output gradient g (dvc_enc_wgrad; taps 343: the stem, dvc_enc_stem_wgrad)."""
    _enc_5d("enc_wgrad: x and g", x, g)
    B, cin, H, W, D = x.shape
    cout = int(g.shape[1])
    if taps not in (1, 27, _lib.ENC_STEM_TAPS) or stride not in (1, 2) or prologue not in (0, 1, 2) or g.shape[0] != B \
            or tuple(g.shape[2:]) != enc_out_volume((H, W, D), stride):
        raise ValueError(f"enc_wgrad: taps {taps}, stride {stride}, prologue {prologue}, x {tuple(x.shape)}, g "
                         f"{tuple(g.shape)}")
    if prologue == _lib.ENC_NORM_RELU:
        if scale_shift is None or tuple(scale_shift.shape) != (B, cin, 2):
            raise ValueError("enc_wgrad: prologue 2 needs a (B, cin, 2) scale_shift")
        _need_cuda(scale_shift)
        _conv_operand(scale_shift, "enc_wgrad: scale_shift")
    L = lib()
    stem = taps == _lib.ENC_STEM_TAPS
    nbytes = L.dvc_enc_stem_wgrad_workspace_bytes(stride, B, H, W, D) if stem and cin == 1 and cout == _lib.ENC_STEM_COUT \
        else 0 if stem else L.dvc_enc_wgrad_workspace_bytes(taps, stride, cin, cout, B, H, W, D)
    if nbytes == 0:
        raise NotImplementedError(f"enc_wgrad: taps={taps} cin={cin} cout={cout} is outside the kernel's shapes")
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    k = {1: 1, 27: 3}.get(taps, 7)
    dw = torch.empty((cout, cin, k, k, k), dtype=torch.float32, device=x.device)
    if stem:
        check(L.dvc_enc_stem_wgrad(_ptr(x), _ptr(g), _ptr(dw), _ptr(ws), stride, B, H, W, D, dtype, _stream(x)),
              "enc_stem_wgrad")
    else:
        check(L.dvc_enc_wgrad(_ptr(x), None if scale_shift is None else _ptr(scale_shift), prologue, _ptr(g), _ptr(dw),
                              _ptr(ws), taps, stride, cin, cout, B, H, W, D, dtype, _stream(x)), "enc_wgrad")
    return dw
