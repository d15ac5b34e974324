"""torch.library registrations of the correlation ops.

The drop-in blocks (corr_block.py) call these, so the hot path is visible to
the PyTorch dispatcher as named operators with shape functions:

    dvccorr::build(q, t, ...)                    -> corr pyramid (B, Nq, row_stride)   corr.py:141-167
    dvccorr::lookup(corr, coords, ...)           -> (B, L*(2r+1)^3, Nq) f32            corr.py:169-208
    dvccorr::lookup_fused(q, t, coords, ...)     -> (B, L*(2r+1)^3, Nq) f32            corr_otf.py:96-237
    dvccorr::lookup_fused_proj(q, t, coords, w, b, ...) -> (B, 96, Nq) f32 = relu(convc1(lookup_fused))
                                                 (bf16 / fp16 operands, or fp32 with the exact hi / lo weight pack)
                                                                                       + update.py:246
    dvccorr::corr_backward(q, t, coords, g, ...) -> (d fmap1 (B, C, Nq), d fmap2)      autograd of corr.py:141-208
    dvccorr::lookup_convc1_ad(fmap1, fmap2, weight, bias, corr?, q, t, coords, packed_w, ...)
        relu(convc1(lookup)) differentiable (update.py:246): the fused kernel forward, the backward
        recomputes the lookup and feeds W^T (dy * relu') to dvccorr::corr_backward
    dvccorr::lookup_ad(fmap1, fmap2, corr?, q, t, coords, ...)
        the lookup as a differentiable op: fmap1 / fmap2 are its gradient carriers
        (the values it reads are the packed q / t / corr built from them), and the
        registered autograd formula is dvccorr::corr_backward.  Coordinates get no
        gradient (RAFTDVC.forward detaches them, raft_dvc.py:441).

    dvccorr::sep_gru(h, x, packed, dtype)        -> h after SepConvGRU3D's three passes  update.py:178-199
                                                 (forward only: no autograd formula is registered)
    dvccorr::conv3(src0, src1?, packed, dst, dst_offset, cout, relu, dtype)   writes a channel slice of dst:
                                                 3 x 3 x 3 conv of cat[src0, src1] + bias (+ ReLU)   update.py:226-251
    dvccorr::conv7_flow(flow, packed, dst, dtype)    dst = relu(convf1(flow))                         update.py:225, 247

    dvccorr::conv3_ad(x, x2?, weight, bias, relu, dtype) -> y   the same layer as a differentiable op (update.py:226-251);
        its registered backward is dvccorr::conv3_grad_prep(grad_y, y?, relu) -> (g, db), dvccorr::conv3_wgrad(x, x2?,
        g, dtype) -> dW and dvccorr::conv3 on g with the transposed, flipped weights of dvccorr::conv3_pack_dgrad(weight,
        dtype) (a cached pack, no compute)

    dvccorr::conv7_ad(flow, weight, bias, dtype) -> y   relu(convf1(flow)) as a differentiable op (update.py:225, 247):
        forward dvccorr::conv7_flow's kernel into a new tensor; its registered backward is dvccorr::conv3_grad_prep
        (mask from y, db) and dvccorr::conv7_wgrad(flow, g, dtype) -> dW (64, 3, 7, 7, 7).  The model detaches the flow
        (raft_dvc.py:441); a flow that does require grad gets torch.nn.grad.conv3d_input of g in float32 (slow path)

    dvccorr::sep_gru_ad(h, x, weights[18], dtype) -> (h_out, saved)   SepConvGRU3D.forward as a differentiable op
        (update.py:167-199): the training forward keeps z, r, q of the three passes and the two intermediate hidden
        states in `saved` (non-differentiable); its registered backward runs, per pass and in reverse,
        dvccorr::gru_grad_prep(g, z, q, h) -> (a_q, a_z, dh0, db_q, db_z), dvccorr::gru_dgrad(a_q, a_z, h, r, packed, dh,
        dx?, axis, dx_add, dtype) -> (a_r, db_r) (dh and dx updated in place) with the weights of
        dvccorr::gru_pack_dgrad(weights, dtype) (a cached pack) and dvccorr::gru_wgrad(h, x, r, a_z, a_r, a_q, axis,
        dtype) -> dW of the pass's three convolutions

    dvccorr::enc_stem(x, packed, y, partials?, stride, dtype)   y = conv1(x) + bias, raw         extractor.py:168, 239
    dvccorr::enc_conv(x, scale_shift?, prologue, packed, y, y2?, partials?, taps, stride, dtype)   a bottleneck
        convolution, the strided shortcut or conv2 with the producer's norm + ReLU applied on load   extractor.py:93-139
    dvccorr::enc_conv_new(x, scale_shift?, prologue, packed, cout, split, taps, stride, dtype) -> (y, y2)   the same
        into new tensors (conv2; split >= 0: the context encoder's tanh / ReLU halves, extractor.py:298-300)
    dvccorr::enc_stats(partials, scale_shift, taps, stride, ovol, eps)   InstanceNorm3d's (scale, shift) per (b, c)
    dvccorr::enc_residual(c3, ss3?, shortcut, ss4?, mode, out)   out = relu(norm3(c3) + shortcut)   extractor.py:131-137
        (all forward only: no autograd formula is registered)

Every op runs the HIP kernels of libdvccorr.so through ops.py (no CPU
fallback); the fake (meta) implementations only compute output shapes, so the
ops trace under torch.compile / FakeTensorMode and torch.library.opcheck.
`torch.utils.checkpoint(block, coords, use_reentrant=False)` (the reference's
checkpoint_corr path, raft_dvc.py:446-448) recomputes dvccorr::lookup_ad in the
backward pass.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
from torch import Tensor

from . import ops
from ._lib import layout

_F32 = torch.float32


def _n3(radius: int) -> int:
    return (2 * radius + 1) ** 3


@torch.library.custom_op("dvccorr::build", mutates_args=())
def build(packed_q: Tensor, packed_t: Tensor, C: int, H: int, W: int, D: int, num_levels: int,
          dtype: int) -> Tensor:
    return ops.build(packed_q, packed_t, C, H, W, D, num_levels, dtype, dtype)


@build.register_fake
def _(packed_q, packed_t, C, H, W, D, num_levels, dtype):
    # same metadata as ops.alloc_corr: a view past DVC_CORR_GUARD_BYTES of leading zeros
    lay = layout(H, W, D, num_levels, C)
    B, Nq, _ = packed_q.shape
    dt = ops._TORCH_DT[dtype]
    g = ops.GUARD_BYTES // torch.tensor([], dtype=dt).element_size()
    n = B * Nq * lay.row_stride
    return packed_q.new_empty((n + 2 * g,), dtype=dt)[g:g + n].view(B, Nq, lay.row_stride)


@torch.library.custom_op("dvccorr::lookup", mutates_args=())
def lookup(corr: Tensor, coords: Tensor, H: int, W: int, D: int, num_levels: int, radius: int, legacy: bool,
           dtype: int) -> Tensor:
    return ops.lookup(corr, coords, H, W, D, num_levels, radius, legacy, dtype)


@lookup.register_fake
def _(corr, coords, H, W, D, num_levels, radius, legacy, dtype):
    B, Nq, _ = corr.shape
    return corr.new_empty((B, num_levels * _n3(radius), Nq), dtype=_F32)


@torch.library.custom_op("dvccorr::lookup_fused", mutates_args=())
def lookup_fused(packed_q: Tensor, packed_t: Tensor, coords: Tensor, C: int, H: int, W: int, D: int,
                 num_levels: int, radius: int, legacy: bool, dtype: int) -> Tensor:
    return ops.lookup_fused(packed_q, packed_t, coords, C, H, W, D, num_levels, radius, legacy, dtype)


@lookup_fused.register_fake
def _(packed_q, packed_t, coords, C, H, W, D, num_levels, radius, legacy, dtype):
    B, Nq, _ = packed_q.shape
    return packed_q.new_empty((B, num_levels * _n3(radius), Nq), dtype=_F32)


@torch.library.custom_op("dvccorr::lookup_fused_proj", mutates_args=())
def lookup_fused_proj(packed_q: Tensor, packed_t: Tensor, coords: Tensor, packed_w: Tensor, bias: Tensor, C: int,
                      H: int, W: int, D: int, num_levels: int, radius: int, legacy: bool, dtype: int) -> Tensor:
    return ops.lookup_fused_proj(packed_q, packed_t, coords, packed_w, bias, C, H, W, D, num_levels, radius, legacy,
                                 dtype)


@lookup_fused_proj.register_fake
def _(packed_q, packed_t, coords, packed_w, bias, C, H, W, D, num_levels, radius, legacy, dtype):
    B, Nq, _ = packed_q.shape
    return packed_q.new_empty((B, 96, Nq), dtype=_F32)


@torch.library.custom_op("dvccorr::corr_backward", mutates_args=())
def corr_backward(packed_q: Tensor, packed_t: Tensor, coords: Tensor, grad_out: Tensor, C: int, H: int, W: int,
                  D: int, num_levels: int, radius: int, legacy: bool, dtype: int) -> tuple[Tensor, Tensor]:
    return ops.corr_backward(packed_q, packed_t, coords, grad_out, C, H, W, D, num_levels, radius, legacy, dtype)


@corr_backward.register_fake
def _(packed_q, packed_t, coords, grad_out, C, H, W, D, num_levels, radius, legacy, dtype):
    B, Nq, _ = packed_q.shape
    return (packed_q.new_empty((B, C, Nq), dtype=_F32), packed_q.new_empty((B, C, H, W, D), dtype=_F32))


@torch.library.custom_op("dvccorr::lookup_ad", mutates_args=())
def lookup_ad(fmap1: Tensor, fmap2: Tensor, corr: Optional[Tensor], packed_q: Tensor, packed_t: Tensor,
              coords: Tensor, C: int, H: int, W: int, D: int, num_levels: int, radius: int, legacy: bool,
              dtype: int) -> Tensor:
    if corr is not None:
        return ops.lookup(corr, coords, H, W, D, num_levels, radius, legacy, dtype)
    return ops.lookup_fused(packed_q, packed_t, coords, C, H, W, D, num_levels, radius, legacy, dtype)


@lookup_ad.register_fake
def _(fmap1, fmap2, corr, packed_q, packed_t, coords, C, H, W, D, num_levels, radius, legacy, dtype):
    B, Nq, _ = packed_q.shape
    return packed_q.new_empty((B, num_levels * _n3(radius), Nq), dtype=_F32)


def _lookup_ad_setup(ctx, inputs, output):
    fmap1, fmap2, _corr, q, t, coords, C, H, W, D, L, r, legacy, dtype = inputs
    ctx.save_for_backward(q, t, coords)
    ctx.geo = (C, H, W, D, L, r, legacy, dtype)
    ctx.fmap_meta = (tuple(fmap1.shape), fmap1.dtype, tuple(fmap2.shape), fmap2.dtype)


def _lookup_ad_backward(ctx, grad_out):
    q, t, coords = ctx.saved_tensors
    C, H, W, D, L, r, legacy, dtype = ctx.geo
    s1, dt1, s2, dt2 = ctx.fmap_meta
    d1, d2 = corr_backward(q, t, coords, grad_out.contiguous(), C, H, W, D, L, r, legacy, dtype)
    return (d1.view(s1).to(dt1), d2.view(s2).to(dt2)) + (None,) * 12


torch.library.register_autograd("dvccorr::lookup_ad", _lookup_ad_backward, setup_context=_lookup_ad_setup)


@torch.library.custom_op("dvccorr::lookup_convc1_ad", mutates_args=())
def lookup_convc1_ad(fmap1: Tensor, fmap2: Tensor, weight: Tensor, bias: Tensor, corr: Optional[Tensor],
                     packed_q: Optional[Tensor], packed_t: Optional[Tensor], coords: Tensor, packed_w: Tensor, C: int,
                     H: int, W: int,
                     D: int, num_levels: int, radius: int, legacy: bool, dtype: int, store_dtype: int) -> Tensor:
    """relu(convc1(lookup(coords))) (update.py:246 after corr.py:169-208) as a differentiable op.  The forward is the
    fused kernel (materialised: dvc_corr_lookup_proj on `corr`; on the fly: dvc_corr_lookup_fused_proj on the packed
    operands), so the L*(2r+1)^3-channel lookup tensor is neither written nor saved for the backward: the
    autograd context keeps the (B, 96, Nq) output and the coordinates only.  fmap1 / fmap2 / weight / bias are the
    gradient carriers (packed_w is weight's packed fp16 image)."""
    if corr is not None:
        return ops.lookup_proj(corr, coords, packed_w, bias, H, W, D, num_levels, radius, legacy, store_dtype)
    return ops.lookup_fused_proj(packed_q, packed_t, coords, packed_w, bias, C, H, W, D, num_levels, radius, legacy,
                                 dtype)


@lookup_convc1_ad.register_fake
def _(fmap1, fmap2, weight, bias, corr, packed_q, packed_t, coords, packed_w, C, H, W, D, num_levels, radius, legacy,
      dtype, store_dtype):
    B, _, Nq = coords.shape
    return coords.new_empty((B, 96, Nq), dtype=_F32)


def _lookup_convc1_setup(ctx, inputs, output):
    fmap1, fmap2, weight, bias, corr, q, t, coords, _pw, C, H, W, D, L, r, legacy, dtype, sdt = inputs
    ctx.save_for_backward(q, t, coords, weight, output, corr)
    ctx.geo = (C, H, W, D, L, r, legacy, dtype, sdt)
    ctx.meta = (tuple(fmap1.shape), fmap1.dtype, tuple(fmap2.shape), fmap2.dtype, tuple(bias.shape), bias.dtype)


def _lookup_convc1_backward(ctx, grad_out):
    """With y = relu(W x + b) per query (x = the lookup's L*(2r+1)^3 values): gy = dL/dy * [y > 0];
    dW = sum_q gy x^T, db = sum_q gy, dx = W^T gy, and dx goes through dvccorr::corr_backward to the fmaps.
    x is recomputed by the plain lookup kernel (one fp32 pass, freed after dW) instead of being saved by the
    forward: the Trainer's twelve iterations keep 12 x (B, 96, Nq) instead of 12 x (B, L*(2r+1)^3, Nq)."""
    q, t, coords, weight, out, corr = ctx.saved_tensors
    C, H, W, D, L, r, legacy, dtype, sdt = ctx.geo
    s1, dt1, s2, dt2, sb, dtb = ctx.meta
    gy = grad_out.contiguous() * (out > 0)
    x = (ops.lookup(corr, coords, H, W, D, L, r, legacy, sdt) if corr is not None else
         ops.lookup_fused(q, t, coords, C, H, W, D, L, r, legacy, dtype))         # (B, K, Nq) fp32
    w2 = weight.detach().reshape(weight.shape[0], -1).float()                         # (96, K)
    dw = torch.einsum("bon,bkn->ok", gy, x).reshape(weight.shape).to(weight.dtype)
    del x
    db = gy.sum(dim=(0, 2)).reshape(sb).to(dtb)
    d1 = d2 = None
    if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:   # (the block's fmaps require grad: q / t were kept)
        dx = torch.einsum("ok,bon->bkn", w2, gy).contiguous()
        d1, d2 = corr_backward(q, t, coords, dx, C, H, W, D, L, r, legacy, dtype)
        d1, d2 = d1.view(s1).to(dt1), d2.view(s2).to(dt2)
    return (d1, d2, dw, db) + (None,) * 14


torch.library.register_autograd("dvccorr::lookup_convc1_ad", _lookup_convc1_backward,
                                setup_context=_lookup_convc1_setup)

@torch.library.custom_op("dvccorr::sep_gru", mutates_args=())
def sep_gru(h: Tensor, x: Tensor, packed: Tensor, dtype: int) -> Tensor:
    return ops.sep_gru(h, x, packed, dtype)


@sep_gru.register_fake
def _(h, x, packed, dtype):
    return h.new_empty(h.shape, dtype=_F32)


# the update block's plain convolutions: they write a preallocated destination (a channel slice of it for conv3)
@torch.library.custom_op("dvccorr::conv3", mutates_args=("dst",))
def conv3(src0: Tensor, src1: Optional[Tensor], packed: Tensor, dst: Tensor, dst_offset: int, cout: int, relu: bool,
          dtype: int) -> None:
    ops.conv3(src0, src1, packed, dst, dst_offset, cout, relu, dtype)


@conv3.register_fake
def _(src0, src1, packed, dst, dst_offset, cout, relu, dtype):
    return None


@torch.library.custom_op("dvccorr::conv7_flow", mutates_args=("dst",))
def conv7_flow(flow: Tensor, packed: Tensor, dst: Tensor, dtype: int) -> None:
    ops.conv7_flow(flow, packed, dst, dtype)


@conv7_flow.register_fake
def _(flow, packed, dst, dtype):
    return None


# the encoders' forward (dvccorr.Encoder, csrc/encoder.hip): every kernel writes preallocated tensors
@torch.library.custom_op("dvccorr::enc_stem", mutates_args=("y", "partials"))
def enc_stem(x: Tensor, packed: Tensor, y: Tensor, partials: Optional[Tensor], stride: int, dtype: int) -> None:
    ops.enc_stem(x, packed, y, partials, stride, dtype)


@enc_stem.register_fake
def _(x, packed, y, partials, stride, dtype):
    return None


@torch.library.custom_op("dvccorr::enc_conv", mutates_args=("y", "y2", "partials"))
def enc_conv(x: Tensor, scale_shift: Optional[Tensor], prologue: int, packed: Tensor, y: Tensor, y2: Optional[Tensor],
             partials: Optional[Tensor], taps: int, stride: int, dtype: int) -> None:
    ops.enc_conv(x, scale_shift, prologue, packed, y, y2, partials, taps, stride, dtype)


@enc_conv.register_fake
def _(x, scale_shift, prologue, packed, y, y2, partials, taps, stride, dtype):
    return None


@torch.library.custom_op("dvccorr::enc_stats", mutates_args=("scale_shift",))
def enc_stats(partials: Tensor, scale_shift: Tensor, taps: int, stride: int, ovol: Sequence[int], eps: float) -> None:
    ops.enc_stats(partials, scale_shift, taps, stride, tuple(ovol), eps)


@enc_stats.register_fake
def _(partials, scale_shift, taps, stride, ovol, eps):
    return None


@torch.library.custom_op("dvccorr::enc_residual", mutates_args=("out",))
def enc_residual(c3: Tensor, ss3: Optional[Tensor], shortcut: Tensor, ss4: Optional[Tensor], mode: int,
                 out: Tensor) -> None:
    ops.enc_residual(c3, ss3, shortcut, ss4, mode, out)


@enc_residual.register_fake
def _(c3, ss3, shortcut, ss4, mode, out):
    return None


@torch.library.custom_op("dvccorr::enc_conv_new", mutates_args=())
def enc_conv_new(x: Tensor, scale_shift: Optional[Tensor], prologue: int, packed: Tensor, cout: int, split: int,
                 taps: int, stride: int, dtype: int) -> tuple[Tensor, Tensor]:
    """dvccorr::enc_conv into new tensors (the encoder's conv2, whose result is returned to the caller): (y, empty)
    for split < 0, else (tanh of channels [0, split), ReLU of the rest)."""
    ovol = ops.enc_out_volume(x.shape[2:], stride)
    y = torch.empty((x.shape[0], cout if split < 0 else split) + ovol, dtype=_F32, device=x.device)
    y2 = torch.empty((x.shape[0], 0 if split < 0 else cout - split) + ovol, dtype=_F32, device=x.device)
    ops.enc_conv(x, scale_shift, prologue, packed, y, None if split < 0 else y2, None, taps, stride, dtype)
    return y, y2


@enc_conv_new.register_fake
def _(x, scale_shift, prologue, packed, cout, split, taps, stride, dtype):
    ovol = ops.enc_out_volume(x.shape[2:], stride)
    return (x.new_empty((x.shape[0], cout if split < 0 else split) + ovol, dtype=_F32),
            x.new_empty((x.shape[0], 0 if split < 0 else cout - split) + ovol, dtype=_F32))


# ---------------------------------------------------------------------------------------------------------------
# a differentiable 3 x 3 x 3 layer (dvccorr.conv3x3x3_ad): forward k_conv3_mfma, backward csrc/conv3_grad.hip
# ---------------------------------------------------------------------------------------------------------------
_conv3_ad_packs = None


def _conv3_packs():
    """The module-level pack cache of conv3_ad: entries keyed (kind, weight / bias objects, precision), valid for the
    tensors' version counters and storage (update._PackCache), so calls between optimiser steps do not re-pack."""
    global _conv3_ad_packs
    if _conv3_ad_packs is None:
        from .update import _PackCache
        _conv3_ad_packs = _PackCache()
    return _conv3_ad_packs


_CONV3_AD_MAX_PACKS = 64   # an entry keeps its weights alive: a cache past this many layers starts over


def _conv3_packed(weight: Tensor, bias: Tensor, dtype: int) -> Tensor:
    if len(_conv3_packs()._entries) > _CONV3_AD_MAX_PACKS:
        _conv3_packs()._entries.clear()
    return _conv3_packs().get(("fwd", id(weight), id(bias), dtype), (weight, bias),
                              lambda: ops.conv3_pack(weight, bias, dtype))


@torch.library.custom_op("dvccorr::conv3_pack_dgrad", mutates_args=())
def conv3_pack_dgrad(weight: Tensor, dtype: int) -> Tensor:
    """ops.conv3_pack_dgrad through the pack cache: the input gradient's weights, as an operator so that the backward
    of dvccorr::conv3_ad traces."""
    return _conv3_packs().get(("dgrad", id(weight), dtype), (weight,), lambda: ops.conv3_pack_dgrad(weight, dtype))


@conv3_pack_dgrad.register_fake
def _(weight, dtype):
    # dvc_conv3_packed_bytes(cout, cin, dtype): the layer with the channel counts swapped
    tiles, chunks = (weight.shape[1] + 15) // 16, (weight.shape[0] + 31) // 32
    nt = tiles if tiles <= 2 else 4 if tiles <= 4 else 5 if tiles == 5 else 8
    return weight.new_empty((chunks * 27 * nt * (2 if dtype == ops.DVC_F32 else 1) * 256 + 16 * nt,), dtype=_F32)


@torch.library.custom_op("dvccorr::conv3_ad", mutates_args=())
def conv3_ad(x: Tensor, x2: Optional[Tensor], weight: Tensor, bias: Tensor, relu: bool, dtype: int) -> Tensor:
    """conv3x3x3(cat[x, x2]) + bias (+ ReLU) as a differentiable op: packs the weights (cached), allocates y and runs
    dvc_conv3.  x, x2, weight and bias carry gradients."""
    x = ops._f32c(x)
    x2 = None if x2 is None else ops._f32c(x2)
    y = torch.empty((x.shape[0], weight.shape[0]) + tuple(x.shape[2:]), dtype=_F32, device=x.device)
    ops.conv3(x, x2, _conv3_packed(weight, bias, dtype), y, 0, int(weight.shape[0]), relu, dtype)
    return y


@conv3_ad.register_fake
def _(x, x2, weight, bias, relu, dtype):
    return x.new_empty((x.shape[0], weight.shape[0]) + tuple(x.shape[2:]), dtype=_F32)


@torch.library.custom_op("dvccorr::conv3_grad_prep", mutates_args=())
def conv3_grad_prep(grad_y: Tensor, y: Optional[Tensor], relu: bool) -> tuple[Tensor, Tensor]:
    g, db = ops.conv3_grad_prep(grad_y, y, relu)
    # an operator may not return an input: without ReLU the caller keeps grad_y (no copy) and g is empty
    return (g if relu else grad_y.new_empty(0)), db


@conv3_grad_prep.register_fake
def _(grad_y, y, relu):
    return (grad_y.new_empty(grad_y.shape if relu else (0,), dtype=_F32), grad_y.new_empty((grad_y.shape[1],), dtype=_F32))


@torch.library.custom_op("dvccorr::conv3_wgrad", mutates_args=())
def conv3_wgrad(x: Tensor, x2: Optional[Tensor], g: Tensor, dtype: int) -> Tensor:
    return ops.conv3_wgrad(x, x2, g, dtype)


@conv3_wgrad.register_fake
def _(x, x2, g, dtype):
    cin = x.shape[1] + (0 if x2 is None else x2.shape[1])
    return x.new_empty((g.shape[1], cin, 3, 3, 3), dtype=_F32)


def _conv3_ad_setup(ctx, inputs, output):
    x, x2, weight, bias, relu, dtype = inputs
    ctx.save_for_backward(x, x2, weight, output if relu else None)
    ctx.cfg = (bool(relu), int(dtype))
    ctx.meta = (x.dtype, None if x2 is None else x2.dtype, weight.dtype, tuple(bias.shape), bias.dtype)


def _conv3_ad_backward(ctx, grad_y):
    """g = dL/dy [y > 0] (the mask from the op's own stored output) and db in one pass (dvccorr::conv3_grad_prep);
    dW on k_conv3_wgrad (dvccorr::conv3_wgrad); d cat[x, x2] as one dvccorr::conv3 launch of g with the transposed,
    flipped weights, dx and dx2 its two channel ranges.  Whatever needs_input_grad does not ask for is skipped."""
    if grad_y.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("dvccorr.conv3x3x3_ad has no double backward")
    x, x2, weight, y = ctx.saved_tensors
    relu, dtype = ctx.cfg
    dtx, dtx2, dtw, sb, dtb = ctx.meta
    need_x, need_x2, need_w, need_b = ctx.needs_input_grad[:4]
    dx = dx2 = dw = db = None
    if not (need_x or need_x2 or need_w or need_b):
        return (None,) * 6
    grad_y = ops._f32c(grad_y)
    g, db_ = conv3_grad_prep(grad_y, y, relu)
    if not relu:
        g = grad_y
    if need_b:
        db = db_.reshape(sb).to(dtb)
    if need_w:
        dw = conv3_wgrad(ops._f32c(x), None if x2 is None else ops._f32c(x2), g, dtype).to(dtw)
    if need_x or need_x2:
        c0, cin, cout = int(x.shape[1]), int(weight.shape[1]), int(weight.shape[0])
        dcat = torch.empty((g.shape[0], cin) + tuple(g.shape[2:]), dtype=_F32, device=g.device)
        conv3(g, None, conv3_pack_dgrad(weight, dtype), dcat, 0, cin, False, dtype)
        if need_x:
            dx = dcat[:, :c0].to(dtx)
        if need_x2:
            dx2 = dcat[:, c0:].to(dtx2)
    return dx, dx2, dw, db, None, None


torch.library.register_autograd("dvccorr::conv3_ad", _conv3_ad_backward, setup_context=_conv3_ad_setup)


# ---------------------------------------------------------------------------------------------------------------
# a differentiable encoder.convf1 (dvccorr.conv7x7x7_flow_ad): forward k_conv7_flow, backward csrc/conv7_grad.hip
# ---------------------------------------------------------------------------------------------------------------
@torch.library.custom_op("dvccorr::conv7_wgrad", mutates_args=())
def conv7_wgrad(flow: Tensor, g: Tensor, dtype: int) -> Tensor:
    return ops.conv7_wgrad(flow, g, dtype)


@conv7_wgrad.register_fake
def _(flow, g, dtype):
    return flow.new_empty((g.shape[1], 3, 7, 7, 7), dtype=_F32)


@torch.library.custom_op("dvccorr::conv7_ad", mutates_args=())
def conv7_ad(flow: Tensor, weight: Tensor, bias: Tensor, dtype: int) -> Tensor:
    """relu(conv7x7x7(flow) + bias) as a differentiable op: packs the weights (cached), allocates y and runs
    dvc_conv7_flow.  weight and bias carry gradients (flow too, on a slow path)."""
    flow = ops._f32c(flow)
    if len(_conv3_packs()._entries) > _CONV3_AD_MAX_PACKS:
        _conv3_packs()._entries.clear()
    packed = _conv3_packs().get(("fwd7", id(weight), id(bias), dtype), (weight, bias),
                                lambda: ops.conv7_flow_pack(weight, bias, dtype))
    y = torch.empty((flow.shape[0], weight.shape[0]) + tuple(flow.shape[2:]), dtype=_F32, device=flow.device)
    ops.conv7_flow(flow, packed, y, dtype)
    return y


@conv7_ad.register_fake
def _(flow, weight, bias, dtype):
    return flow.new_empty((flow.shape[0], weight.shape[0]) + tuple(flow.shape[2:]), dtype=_F32)


def _conv7_ad_setup(ctx, inputs, output):
    flow, weight, bias, dtype = inputs
    ctx.save_for_backward(flow, weight, output)
    ctx.dtype = int(dtype)
    ctx.meta = (flow.dtype, weight.dtype, tuple(bias.shape), bias.dtype)


def _conv7_ad_backward(ctx, grad_y):
    """g = dL/dy [y > 0] (the mask from the op's own stored output) and db in one pass (dvccorr::conv3_grad_prep); dW
    on k_conv7_wgrad (dvccorr::conv7_wgrad).  A flow that requires grad (the model's never does) gets
    torch.nn.grad.conv3d_input of g in float32.  Whatever needs_input_grad does not ask for is skipped."""
    if grad_y.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("dvccorr.conv7x7x7_flow_ad has no double backward")
    flow, weight, y = ctx.saved_tensors
    dtf, dtw, sb, dtb = ctx.meta
    need_f, need_w, need_b = ctx.needs_input_grad[:3]
    df = dw = db = None
    if not (need_f or need_w or need_b):
        return (None,) * 4
    g, db_ = conv3_grad_prep(ops._f32c(grad_y), y, True)
    if need_b:
        db = db_.reshape(sb).to(dtb)
    if need_w:
        dw = conv7_wgrad(ops._f32c(flow), g, ctx.dtype).to(dtw)
    if need_f:
        with torch.autocast("cuda", enabled=False):
            df = torch.nn.grad.conv3d_input(flow.shape, weight.detach().float(), g, padding=3).to(dtf)
    return df, dw, db, None


torch.library.register_autograd("dvccorr::conv7_ad", _conv7_ad_backward, setup_context=_conv7_ad_setup)


# ---------------------------------------------------------------------------------------------------------------
# a differentiable SepConvGRU3D (dvccorr.sep_conv_gru_ad): forward k_sep_gru_pass<SAVE>, backward csrc/gru_grad.hip
# ---------------------------------------------------------------------------------------------------------------
_GRU_NAMES = tuple(f"conv{g}_{ax}.{kind}" for ax in "hwd" for g in "zrq" for kind in ("weight", "bias"))


def _gru_dict(weights):
    if len(weights) != len(_GRU_NAMES):
        raise ValueError(f"sep_gru_ad: {len(weights)} weight tensors; SepConvGRU3D has {len(_GRU_NAMES)} "
                         "(update.GRU_WEIGHT_NAMES order)")
    return dict(zip(_GRU_NAMES, weights))


def _gru_packed(weights, dtype: int, kind: str, pack) -> Tensor:
    if len(_conv3_packs()._entries) > _CONV3_AD_MAX_PACKS:
        _conv3_packs()._entries.clear()
    return _conv3_packs().get((kind, id(weights[0]), dtype), weights, lambda: pack(_gru_dict(weights), dtype))


@torch.library.custom_op("dvccorr::gru_pack_dgrad", mutates_args=())
def gru_pack_dgrad(weights: Sequence[Tensor], dtype: int) -> Tensor:
    """ops.gru_pack_dgrad through the pack cache (an optimiser step re-packs), as an operator so that the backward of
    dvccorr::sep_gru_ad traces."""
    return _gru_packed(list(weights), dtype, "gru_dgrad", ops.gru_pack_dgrad)


@gru_pack_dgrad.register_fake
def _(weights, dtype):
    # 3 x dvc_gru_dgrad_packed_bytes: (3 + 6) chunks x 5 taps x 16 tiles of 1 KB fragments, two pieces for fp32
    return weights[0].new_empty((3, 720 * (2 if dtype == ops.DVC_F32 else 1) * 256), dtype=_F32)


@torch.library.custom_op("dvccorr::sep_gru_ad", mutates_args=())
def sep_gru_ad(h: Tensor, x: Tensor, weights: Sequence[Tensor], dtype: int) -> tuple[Tensor, Tensor]:
    """SepConvGRU3D.forward(h, x) as a differentiable op: (h_out, saved).  saved (11, B, 96, H, W, D) float32 holds z, r,
    q of the three passes and the hidden states after the h and w passes for the backward: 11 x 96 x B H W D floats,
    138 MB at 32^3.  h, x and the eighteen weights carry gradients; saved does not."""
    packed = _gru_packed(list(weights), dtype, "gru_fwd", ops.gru_pack)
    return ops.sep_gru_save(h, x, packed, dtype)


@sep_gru_ad.register_fake
def _(h, x, weights, dtype):
    return h.new_empty(h.shape, dtype=_F32), h.new_empty((11,) + tuple(h.shape), dtype=_F32)


@torch.library.custom_op("dvccorr::gru_grad_prep", mutates_args=())
def gru_grad_prep(g: Tensor, z: Tensor, q: Tensor, h: Tensor) -> tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    return ops.gru_grad_prep(g, z, q, h)


@gru_grad_prep.register_fake
def _(g, z, q, h):
    e, b = (lambda: g.new_empty(g.shape, dtype=_F32)), (lambda: g.new_empty((g.shape[1],), dtype=_F32))
    return e(), e(), e(), b(), b()


@torch.library.custom_op("dvccorr::gru_dgrad", mutates_args=("dh", "dx"))
def gru_dgrad(aq: Tensor, az: Tensor, h: Tensor, r: Tensor, packed: Tensor, dh: Tensor, dx: Optional[Tensor],
              axis: int, dx_add: bool, dtype: int) -> tuple[Tensor, Tensor]:
    return ops.sep_gru_dgrad(aq, az, h, r, packed[axis], dh, dx, axis, dx_add, dtype)


@gru_dgrad.register_fake
def _(aq, az, h, r, packed, dh, dx, axis, dx_add, dtype):
    return aq.new_empty(aq.shape, dtype=_F32), aq.new_empty((aq.shape[1],), dtype=_F32)


@torch.library.custom_op("dvccorr::gru_wgrad", mutates_args=())
def gru_wgrad(h: Tensor, x: Tensor, r: Tensor, az: Tensor, ar: Tensor, aq: Tensor, axis: int, dtype: int) -> Tensor:
    return ops.gru_wgrad(h, x, r, az, ar, aq, axis, dtype)


@gru_wgrad.register_fake
def _(h, x, r, az, ar, aq, axis, dtype):
    return h.new_empty((3, h.shape[1], h.shape[1] + x.shape[1], 5), dtype=_F32)


def _sep_gru_ad_setup(ctx, inputs, output):
    h, x, weights, dtype = inputs
    _, saved = output
    ctx.mark_non_differentiable(saved)
    ctx.save_for_backward(h, x, saved, *weights)
    ctx.dtype = int(dtype)


def _sep_gru_ad_backward(ctx, grad_h, _grad_saved=None):
    """The three passes in reverse (d, w, h): dh of one pass is the incoming gradient of the pass before it, dx is
    the sum over the passes (the first pass to run stores, the others add).  k_gru_wgrad runs only for an axis with a
    weight that asks, dx is accumulated only when x asks; the bias gradients come with the prep and dgrad kernels."""
    if grad_h.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("dvccorr.sep_conv_gru_ad has no double backward")
    h, x, saved, *weights = ctx.saved_tensors
    need_h, need_x, need_ws = ctx.needs_input_grad[0], ctx.needs_input_grad[1], list(ctx.needs_input_grad[2])
    grads = [None] * len(weights)
    if not (need_h or need_x or any(need_ws)):
        return None, None, grads, None
    dtype = ctx.dtype
    hf, xf = ops._f32c(h), ops._f32c(x)
    packed = gru_pack_dgrad(weights, dtype)
    g = ops._f32c(grad_h)
    dx = torch.empty_like(xf) if need_x else None
    for a in (2, 1, 0):
        if a == 0 and not (need_h or need_x or any(need_ws[:6])):
            break   # nothing upstream of the h pass asks
        h_in = (hf, saved[9], saved[10])[a]
        z, r, q = saved[3 * a], saved[3 * a + 1], saved[3 * a + 2]
        aq, az, dh, dbq, dbz = gru_grad_prep(g, z, q, h_in)
        ar, dbr = gru_dgrad(aq, az, h_in, r, packed, dh, dx, a, a != 2, dtype)
        n = need_ws[6 * a:6 * a + 6]
        if n[0] or n[2] or n[4]:
            dw = gru_wgrad(h_in, xf, r, az, ar, aq, a, dtype)
        for k, db in enumerate((dbz, dbr, dbq)):
            if n[2 * k]:
                grads[6 * a + 2 * k] = dw[k].reshape(weights[6 * a + 2 * k].shape).to(weights[6 * a + 2 * k].dtype)
            if n[2 * k + 1]:
                grads[6 * a + 2 * k + 1] = db.to(weights[6 * a + 2 * k + 1].dtype)
        g = dh
    return (g.to(h.dtype) if need_h else None), (dx.to(x.dtype) if need_x else None), grads, None


torch.library.register_autograd("dvccorr::sep_gru_ad", _sep_gru_ad_backward, setup_context=_sep_gru_ad_setup)


# ---------------------------------------------------------------------------------------------------------------
# the encoders that train (dvccorr.encoder_ad / context_encoder_ad): forward csrc/encoder.hip into new tensors,
# backward csrc/encoder_grad.hip
# ---------------------------------------------------------------------------------------------------------------
@torch.library.custom_op("dvccorr::enc_norm_grad", mutates_args=())
def enc_norm_grad(g: Tensor, x: Optional[Tensor], scale_shift: Optional[Tensor], mask: bool, want_gx: bool,
                  want_db: bool) -> tuple[Tensor, Tensor]:
    """(g_x, db) of ops.enc_norm_grad; what is not asked for is an empty tensor."""
    gx, db = ops.enc_norm_grad(ops._f32c(g), x, scale_shift, mask, want_gx, want_db)
    return (g.new_empty(0) if gx is None else gx), (g.new_empty(0) if db is None else db)


@enc_norm_grad.register_fake
def _(g, x, scale_shift, mask, want_gx, want_db):
    return (g.new_empty(g.shape if want_gx else (0,), dtype=_F32), g.new_empty((g.shape[1],) if want_db else (0,), dtype=_F32))


@torch.library.custom_op("dvccorr::enc_grad_add", mutates_args=())
def enc_grad_add(a: Tensor, b: Optional[Tensor], m: Optional[Tensor]) -> Tensor:
    return ops.enc_grad_add(ops._f32c(a), b, m)


@enc_grad_add.register_fake
def _(a, b, m):
    return a.new_empty(a.shape, dtype=_F32)


@torch.library.custom_op("dvccorr::enc_split_grad", mutates_args=())
def enc_split_grad(g_net: Optional[Tensor], g_ctx: Optional[Tensor], net: Tensor, ctx: Tensor) -> Tensor:
    return ops.enc_split_grad(None if g_net is None else ops._f32c(g_net), None if g_ctx is None else ops._f32c(g_ctx),
                              net, ctx)


@enc_split_grad.register_fake
def _(g_net, g_ctx, net, ctx):
    return net.new_empty((net.shape[0], net.shape[1] + ctx.shape[1]) + tuple(net.shape[2:]), dtype=_F32)


@torch.library.custom_op("dvccorr::enc_pack_dgrad", mutates_args=())
def enc_pack_dgrad(weight: Tensor, dtype: int) -> Tensor:
    """ops.enc_conv_pack_dgrad: the packed weights of an encoder convolution's input gradient (dvccorr.encoder_ad keeps
    them in the weight set's pack cache; this operator packs anew)."""
    return ops.enc_conv_pack_dgrad(weight, dtype)


@enc_pack_dgrad.register_fake
def _(weight, dtype):
    cout, cin, taps = weight.shape[0], weight.shape[1], 27 if weight.shape[2] == 3 else 1
    nt = (cin + 15) // 16
    ntw = 1 if nt == 1 else 2 if (nt == 2 or taps == 27) else 4
    ntp = (nt + ntw - 1) // ntw * ntw
    units = (cout // 8) * 7 if taps == 27 else (cout + 31) // 32
    return weight.new_empty((units * ntp * (3 if dtype == ops.DVC_F32 else 1) * 256 + 16 * ntp,), dtype=_F32)


@torch.library.custom_op("dvccorr::enc_dgrad", mutates_args=())
def enc_dgrad(g: Tensor, packed: Tensor, taps: int, stride: int, cin: int, vol: Sequence[int], dtype: int) -> Tensor:
    return ops.enc_dgrad(g, packed, taps, stride, cin, tuple(vol), dtype)


@enc_dgrad.register_fake
def _(g, packed, taps, stride, cin, vol, dtype):
    return g.new_empty((g.shape[0], cin) + tuple(vol), dtype=_F32)


@torch.library.custom_op("dvccorr::enc_wgrad", mutates_args=())
def enc_wgrad(x: Tensor, scale_shift: Optional[Tensor], prologue: int, g: Tensor, taps: int, stride: int,
              dtype: int) -> Tensor:
    return ops.enc_wgrad(x, scale_shift, prologue, g, taps, stride, dtype)


@enc_wgrad.register_fake
def _(x, scale_shift, prologue, g, taps, stride, dtype):
    k = 1 if taps == 1 else 3 if taps == 27 else 7
    return x.new_empty((g.shape[1], x.shape[1], k, k, k), dtype=_F32)


@torch.library.custom_op("dvccorr::encoder_ad", mutates_args=())
def encoder_ad(x: Tensor, weights: Sequence[Tensor], strides: Sequence[int], instance: bool, split: int, eps: float,
               dtype: int) -> list[Tensor]:
    """An encoder's forward as a differentiable op: [y, y2, *kept].  y is conv2's raw output (split < 0; y2 empty) or
    its tanh half with y2 the ReLU half; kept are the raw convolution outputs, (scale, shift) tables and block outputs
    the backward reads (encoder._ad_kept_names), all float32.  The weights carry gradients; x and kept do not."""
    from . import encoder as E
    return E._ad_forward(x, list(weights), tuple(strides), instance, split, eps, dtype)


@encoder_ad.register_fake
def _(x, weights, strides, instance, split, eps, dtype):
    from . import encoder as E
    return E._ad_fake(x, list(weights), tuple(strides), instance, split)


def _encoder_ad_setup(ctx, inputs, output):
    x, weights, strides, instance, split, eps, dtype = inputs
    ctx.mark_non_differentiable(*output[2:])
    ctx.save_for_backward(x, *weights, *output)
    ctx.cfg = (len(weights), tuple(strides), bool(instance), int(split), float(eps), int(dtype))


def _encoder_ad_backward(ctx, grads):
    from . import encoder as E
    nw, strides, instance, split, eps, dtype = ctx.cfg
    x, *rest = ctx.saved_tensors
    weights, outs = rest[:nw], rest[nw:]
    g_y, g_y2 = grads[0], grads[1]
    if any(g is not None and g.requires_grad for g in (g_y, g_y2)) and torch.is_grad_enabled():
        raise NotImplementedError("dvccorr.encoder_ad has no double backward")
    need = list(ctx.needs_input_grad[1])
    if split < 0:
        g_y2 = None
        if g_y is None:
            return None, [None] * nw, None, None, None, None, None
        g_y = ops._f32c(g_y)
    elif g_y is None and g_y2 is None:
        return None, [None] * nw, None, None, None, None, None
    return None, E._ad_backward(x, weights, strides, instance, split, eps, dtype, outs, g_y, g_y2, need), None, None, \
        None, None, None


torch.library.register_autograd("dvccorr::encoder_ad", _encoder_ad_backward, setup_context=_encoder_ad_setup)


__all__ = ["encoder_ad", "enc_norm_grad", "enc_grad_add", "enc_split_grad", "enc_pack_dgrad", "enc_dgrad", "enc_wgrad", "enc_stem", "enc_conv", "enc_conv_new", "enc_stats", "enc_residual", "conv7_ad", "conv7_wgrad", "sep_gru_ad", "gru_pack_dgrad", "gru_grad_prep", "gru_dgrad", "gru_wgrad", "conv3_ad", "conv3_grad_prep", "conv3_wgrad", "conv3_pack_dgrad", "sep_gru", "conv3", "conv7_flow", "build", "lookup", "lookup_fused", "lookup_fused_proj", "corr_backward", "lookup_ad", "lookup_convc1_ad"]
