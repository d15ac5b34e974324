"""GPU: dvccorr.conv3x3x3_ad, the differentiable 3 x 3 x 3 layer (k_conv3_mfma forward; k_conv3_grad_prep,
k_conv3_wgrad and k_conv3_mfma on the transposed weights backward).

The reference of every gradient is torch autograd through F.conv3d in float64 on the CPU.  Under ReLU the mask comes
from the GPU op's own forward output: grad_y is multiplied by (y_gpu > 0) and the linear layer is differentiated.  An
activation within rounding distance of zero may legitimately land on either side in a 16-bit forward, and a reference
with its own mask would then differ by whole terms (tests/test_gpu_proj_grad.py does the same for the same reason).
Errors are max-normalised per gradient tensor (update_cases.err); the tolerances are the project's standing gradient
tolerances (tests/test_gpu_backward.py): fp32 1e-5, fp16 5e-3, bf16 1e-2."""
from __future__ import annotations

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import prng
import update_cases as uc
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = {"fp32": 1e-5, "fp16": 5e-3, "bf16": 1e-2}
PRECISIONS = ("fp32", "fp16", "bf16")


def _uniform(seed, shape, bound=1.0):
    return torch.from_numpy(prng.uniform(seed, tuple(shape), -bound, bound))


def _layer(seed, c0, c1, cout, B, vol):
    """x, x2 (None when c1 = 0), weight, bias, grad_y of a synthetic layer, CPU float32."""
    cin = c0 + c1
    bound = 1.0 / float(np.sqrt(27 * cin))
    x = _uniform(seed, (B, c0, *vol))
    x2 = _uniform(seed + 1, (B, c1, *vol)) if c1 else None
    return (x, x2, _uniform(seed + 2, (cout, cin, 3, 3, 3), bound), _uniform(seed + 3, (cout,), bound),
            _uniform(seed + 4, (B, cout, *vol)))


def _gpu(x, x2, w, b, gy, relu, precision, need=(True, True, True, True)):
    """y and the gradients (dx, dx2, dw, db) of conv3x3x3_ad on the GPU; entries not asked for are None."""
    import dvccorr
    ts = [None if t is None else t.to(DEV).clone().requires_grad_(n) for t, n in zip((x, x2, w, b), need)]
    y = dvccorr.conv3x3x3_ad(ts[0], ts[2], ts[3], relu=relu, precision=precision, x2=ts[1])
    y.backward(gy.to(DEV))
    return (y.detach(),) + tuple(None if t is None else t.grad for t in ts)


def _ref(x, x2, w, b, g):
    """Gradients of the linear layer conv3d(cat[x, x2], w) + b for the output gradient g: float64 on the CPU."""
    xs = (x if x2 is None else torch.cat([x, x2], dim=1)).double().requires_grad_(True)
    wd, bd = w.double().requires_grad_(True), b.double().requires_grad_(True)
    F.conv3d(xs, wd, bd, padding=1).backward(g.double())
    c0 = x.shape[1]
    return xs.grad[:, :c0], (None if x2 is None else xs.grad[:, c0:]), wd.grad, bd.grad


def _check(x, x2, w, b, gy, relu, precision, what=""):
    y, *got = _gpu(x, x2, w, b, gy, relu, precision)
    g = gy * (y.cpu() > 0) if relu else gy
    errs = {n: uc.err(a, r) for n, a, r in zip(("dx", "dx2", "dw", "db"), got, _ref(x, x2, w, b, g)) if r is not None}
    print(what, precision, "relu" if relu else "linear", {k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) <= TOL[precision], (what, precision, errs)
    return got


# ---------------------------------------------------------------------------------------------------------------
# 1. the reference's own gradients (tests/golden/gen_update_grad_golden.py)
# ---------------------------------------------------------------------------------------------------------------
FWD_TOL = {"fp32": 1e-5, "fp16": 1e-2, "bf16": 1e-2}   # the forward's tolerances (include/dvccorr.h, dvc_conv3)


def _mask_term(x, x2, w, b, g_out, y_ref, y_gpu, precision):
    """The file's ReLU rule applied to stored reference gradients.  They carry the reference's mask [y_ref > 0]; the
    op's carries [y_gpu > 0].  A gradient is linear in the masked output gradient, so the reference under the op's
    mask is the stored one plus the linear layer's float64 gradients (dx, dx2, dw, db) of
    g_out * ([y_gpu > 0] - [y_ref > 0]), which is zero wherever the two masks agree.  The masks may differ only
    where both activations are within the forward's tolerance of zero; anywhere else is a forward error and fails."""
    y_gpu = y_gpu.detach().cpu()
    flip = (y_ref > 0) != (y_gpu > 0)
    lim = FWD_TOL[precision] * float(y_ref.abs().max())
    print(precision, "mask bits that differ:", int(flip.sum()), "of", flip.numel())
    assert not flip.any() or max(float(y_ref[flip].abs().max()), float(y_gpu[flip].abs().max())) <= lim
    return _ref(x, x2, w, b, g_out.double() * ((y_gpu > 0).double() - (y_ref > 0).double()))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_reference_fixture(precision):
    """flow_head = conv2(relu(conv1(net))) as two chained conv3x3x3_ad calls and encoder.conv with its two sources,
    against the reference's autograd results for the losses sum(c * output), c from the fixture's seeds, with the
    ReLU mask taken from the op's own output as everywhere in this file (_mask_term).

    Measured on an MI355X (max over the nine tensors): fp32 5.8e-6, fp16 3.8e-4, bf16 3.2e-3.  One pre-activation of
    encoder.conv in this fixture is +1.4e-4 (of a maximum of 0.147) and becomes -5.9e-5 once the operands are rounded
    to bf16, so the bf16 forward's mask differs from the reference's in that element.  Without _mask_term that one
    element gives d_cor 5.2e-2, d_flo2 6.0e-2 and enc_db 3.1e-1 (a float64 CPU conv of the bf16-rounded operands
    gives the same 0.3125990710660039)."""
    import dvccorr
    ref = {k: torch.from_numpy(v).double() for k, v in load_golden("updgrad_215.npz").items()}
    p, c = uc.params("upd_215"), uc.case("upd_215")
    pd = {n: p[n].to(DEV).clone().requires_grad_(True) for n in p
          if n.startswith("flow_head.") or n.startswith("encoder.conv.")}
    net = c["net"].to(DEV).clone().requires_grad_(True)
    hid = dvccorr.conv3x3x3_ad(net, pd["flow_head.conv1.weight"], pd["flow_head.conv1.bias"], relu=True,
                               precision=precision)
    delta = dvccorr.conv3x3x3_ad(hid, pd["flow_head.conv2.weight"], pd["flow_head.conv2.bias"], precision=precision)
    c_head = torch.from_numpy(prng.uniform(int(ref["seeds"][0]), tuple(delta.shape), -1.0, 1.0))
    (c_head.to(DEV) * delta).sum().backward()
    cor, flo2 = (c[k].to(DEV).clone().requires_grad_(True) for k in ("cor", "flo2"))
    mot = dvccorr.conv3x3x3_ad(cor, pd["encoder.conv.weight"], pd["encoder.conv.bias"], relu=True, precision=precision,
                               x2=flo2)
    c_enc = torch.from_numpy(prng.uniform(int(ref["seeds"][1]), tuple(mot.shape), -1.0, 1.0))
    (c_enc.to(DEV) * mot).sum().backward()
    # the output gradient of flow_head.conv1 is conv2's input gradient of c_head (float64 on the CPU)
    d_hid = _ref(c["hid"], None, p["flow_head.conv2.weight"], p["flow_head.conv2.bias"], c_head)[0]
    h_dx, _, h_dw, h_db = _mask_term(c["net"], None, p["flow_head.conv1.weight"], p["flow_head.conv1.bias"], d_hid,
                                     c["hid"], hid, precision)
    e_dx, e_dx2, e_dw, e_db = _mask_term(c["cor"], c["flo2"], p["encoder.conv.weight"], p["encoder.conv.bias"], c_enc,
                                         c["motion"], mot, precision)
    errs = {"d_net": uc.err(net.grad, ref["d_net"] + h_dx),
            "conv2_dw": uc.err(pd["flow_head.conv2.weight"].grad, ref["conv2_dw"]),
            "conv2_db": uc.err(pd["flow_head.conv2.bias"].grad, ref["conv2_db"]),
            "conv1_dw8": uc.err(pd["flow_head.conv1.weight"].grad[::8], ref["conv1_dw8"] + h_dw[::8]),
            "conv1_db": uc.err(pd["flow_head.conv1.bias"].grad, ref["conv1_db"] + h_db),
            "d_cor": uc.err(cor.grad, ref["d_cor"] + e_dx), "d_flo2": uc.err(flo2.grad, ref["d_flo2"] + e_dx2),
            "enc_dw8": uc.err(pd["encoder.conv.weight"].grad[::8], ref["enc_dw8"] + e_dw[::8]),
            "enc_db": uc.err(pd["encoder.conv.bias"].grad, ref["enc_db"] + e_db)}
    print(precision, {k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) <= TOL[precision], errs


# ---------------------------------------------------------------------------------------------------------------
# 2. channel shapes
# ---------------------------------------------------------------------------------------------------------------
SHAPES = ((96, 0, 128), (96, 32, 80), (128, 0, 3), (64, 0, 32), (33, 0, 17), (40, 24, 21), (1, 0, 1))


@pytest.mark.parametrize("relu", (False, True))
@pytest.mark.parametrize("c0,c1,cout", SHAPES)
def test_channel_shapes(c0, c1, cout, relu):
    layer = _layer(9100 + 10 * SHAPES.index((c0, c1, cout)), c0, c1, cout, 1, (5, 4, 17))
    for precision in PRECISIONS:
        _check(*layer, relu, precision, f"{c0}+{c1}->{cout}")


# ---------------------------------------------------------------------------------------------------------------
# 3. seams of the forward box (dx) and of the weight gradient's K-block and slabs (dW)
# ---------------------------------------------------------------------------------------------------------------
def _seam_volumes():
    from dvccorr import _lib
    fwd = (_lib.CONV3_TH, _lib.CONV3_TW, _lib.CONV3_TD)
    kblk = (_lib.CONV3_WGRAD_KH, _lib.CONV3_WGRAD_KW, _lib.CONV3_WGRAD_KD)
    vols = []
    for ext in (fwd, kblk):
        for axis in range(3):
            for n in (ext[axis] - 1, ext[axis], ext[axis] + 1, 2 * ext[axis] + 1):
                v = [3, 3, 3]
                v[axis] = n
                if tuple(v) not in vols:
                    vols.append(tuple(v))
    return vols


@pytest.mark.parametrize("vol", _seam_volumes(), ids=lambda v: "x".join(map(str, v)))
def test_seams(vol):
    _check(*_layer(9300, 96, 32, 80, 1, vol), True, "fp32", f"seam {vol}")


def test_slab_seams():
    """One volume with fewer K-blocks than the slab rule would like, and one whose K-block count is no multiple of its
    slab count (the last slab is short)."""
    from dvccorr import _lib, ops
    want = -(-_lib.CONV3_WGRAD_TARGET // (8 * 3))            # 128 -> 80: eight ci tiles x three o groups
    nbox, per, nslab = ops.conv3_wgrad_slabs(128, 80, 1, 3, 5, 17)
    assert nbox == 4 < want and (per, nslab) == (1, 4)
    _check(*_layer(9310, 96, 32, 80, 1, (3, 5, 17)), True, "fp32", "few blocks")
    vol = (3, 3, 23 * _lib.CONV3_WGRAD_KD - 5)
    nbox, per, nslab = ops.conv3_wgrad_slabs(128, 80, 1, *vol)
    assert nbox == 23 > want and per == 2 and nslab == 12 and nbox % nslab != 0
    _check(*_layer(9320, 96, 32, 80, 1, vol), False, "fp32", "short last slab")


# ---------------------------------------------------------------------------------------------------------------
# 4. batch
# ---------------------------------------------------------------------------------------------------------------
def test_batch_of_two():
    """Batch elements sum into dW and db and stay apart in dx."""
    x, x2, w, b, gy = _layer(9400, 40, 24, 21, 2, (5, 9, 7))
    for precision in PRECISIONS:
        _check(x, x2, w, b, gy, True, precision, "B=2")
    gy0 = gy.clone()
    gy0[1] = 0                                              # nothing flows back into the second element
    _, dx, dx2, _, _ = _gpu(x, x2, w, b, gy0, False, "fp32")
    assert dx[0].abs().max() > 0 and not dx[1].any() and not dx2[1].any()


# ---------------------------------------------------------------------------------------------------------------
# 5. exact probes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_exact_counts(precision):
    """x = weight = grad_y = 1: dW[o, ci, t] counts the voxels whose tap t lies inside the volume, dx is cout x the
    valid taps of a voxel, db the voxel count.  Small integers: exact in every precision."""
    B, c0, cout, vol = 2, 33, 17, (3, 4, 18)
    ones = lambda *s: torch.ones(*s)   # noqa: E731
    _, dx, _, dw, db = _gpu(ones(B, c0, *vol), None, ones(cout, c0, 3, 3, 3), ones(cout), ones(B, cout, *vol), False,
                            precision)
    inside = [np.array([[0 <= v + k - 1 < n for v in range(n)] for k in range(3)]) for n in vol]   # [tap][voxel]
    taps = np.einsum("ah,bw,cd->abchwd", *inside).astype(np.float64)
    assert torch.equal(dw.cpu().double(), torch.from_numpy(B * taps.sum(axis=(3, 4, 5))).expand(cout, c0, 3, 3, 3))
    assert torch.equal(dx.cpu().double(), torch.from_numpy(cout * taps.sum(axis=(0, 1, 2))).expand(B, c0, *vol))
    assert torch.equal(db.cpu(), torch.full((cout,), float(B * np.prod(vol))))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_dead_relu_gives_zero_gradients(precision):
    x, x2, w, b, gy = _layer(9500, 40, 24, 21, 1, (3, 4, 18))
    y, *grads = _gpu(torch.zeros_like(x), torch.zeros_like(x2), w, -b.abs() - 0.1, gy, True, precision)
    assert not y.any()
    for g in grads:
        assert not g.any()


# ---------------------------------------------------------------------------------------------------------------
# 6. determinism and linearity at the benchmark's size
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_deterministic_and_linear_at_bench_size(precision):
    """Two runs are bit-identical; for fp32 and bf16 (power-of-two scaling commutes with their roundings) grad_y 2^-20
    gives exactly 2^-20 x the gradients."""
    x, x2, w, b, gy = (None if t is None else t.to(DEV) for t in _layer(9600, 96, 32, 80, 1, (32, 32, 32)))
    first = _gpu(x, x2, w, b, gy, True, precision)[1:]
    again = _gpu(x, x2, w, b, gy, True, precision)[1:]
    for a, c in zip(first, again):
        assert torch.equal(a, c)
    if precision != "fp16":
        small = _gpu(x, x2, w, b, gy * 2.0 ** -20, True, precision)[1:]
        for a, c in zip(first, small):
            assert torch.equal(a * 2.0 ** -20, c)


# ---------------------------------------------------------------------------------------------------------------
# 7. needs_input_grad subsets, 8. opcheck, 9. the library path
# ---------------------------------------------------------------------------------------------------------------
def test_needs_input_grad_subsets():
    import dvccorr
    layer = _layer(9700, 40, 24, 21, 1, (4, 4, 4))
    full = _gpu(*layer, True, "fp32")
    _, dx, dx2, dw, db = _gpu(*layer, True, "fp32", need=(False, False, True, False))
    assert dx is None and dx2 is None and db is None and torch.equal(dw, full[3])
    _, dx, dx2, dw, db = _gpu(*layer, True, "fp32", need=(False, True, False, False))
    assert dx is None and dw is None and db is None and torch.equal(dx2, full[2])
    x, x2, w, b, _ = (t.to(DEV).requires_grad_(True) for t in layer)
    with torch.no_grad():
        assert not dvccorr.conv3x3x3_ad(x, w, b, relu=True, x2=x2).requires_grad
    assert not dvccorr.conv3x3x3_ad(x.detach(), w.detach(), b.detach(), x2=x2.detach()).requires_grad
    y = dvccorr.conv3x3x3_ad(x, w, b, relu=True, x2=x2)
    with pytest.raises(NotImplementedError, match="double backward"):
        torch.autograd.grad(y, x, torch.ones_like(y).requires_grad_(True), create_graph=True)


def test_opcheck():
    import dvccorr.library  # noqa: F401
    vol = (4, 4, 4)
    x0 = _uniform(8801, (1, 40, *vol)).to(DEV)
    x1 = _uniform(8802, (1, 19, *vol)).to(DEV)
    w, b = _uniform(8803, (21, 59, 3, 3, 3), 0.03).to(DEV), _uniform(8804, (21,), 0.03).to(DEV)
    gy, y = _uniform(8808, (1, 21, *vol)).to(DEV), _uniform(8809, (1, 21, *vol)).to(DEV)
    rg = lambda t: t.clone().requires_grad_(True)   # noqa: E731
    torch.library.opcheck(torch.ops.dvccorr.conv3_ad.default, (rg(x0), rg(x1), rg(w), rg(b), True, 0))
    torch.library.opcheck(torch.ops.dvccorr.conv3_ad.default, (rg(x0), None, rg(w[:, :40].contiguous()), b, False, 2))
    torch.library.opcheck(torch.ops.dvccorr.conv3_grad_prep.default, (gy, y, True))
    torch.library.opcheck(torch.ops.dvccorr.conv3_grad_prep.default, (gy, None, False))
    torch.library.opcheck(torch.ops.dvccorr.conv3_wgrad.default, (x0, x1, gy, 0))
    torch.library.opcheck(torch.ops.dvccorr.conv3_wgrad.default, (x0, None, gy, 1))
    torch.library.opcheck(torch.ops.dvccorr.conv3_pack_dgrad.default, (w, 0))


def test_fallback_outside_the_kernels_shapes():
    """130 input channels run F.conv3d in float32, still differentiable."""
    _check(*_layer(9900, 130, 0, 8, 1, (5, 4, 17)), True, "fp32", "130->8")
    _check(*_layer(9910, 100, 30, 8, 1, (5, 4, 17)), False, "fp32", "100+30->8")
