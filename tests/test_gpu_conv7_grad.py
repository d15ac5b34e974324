"""GPU: dvccorr.conv7x7x7_flow_ad, the differentiable encoder.convf1 (k_conv7_flow forward; k_conv3_grad_prep and
k_conv7_wgrad backward).

The reference of every gradient is torch autograd through F.conv3d in float64 on the CPU.  The ReLU mask comes from the
GPU op's own forward output, as in tests/test_gpu_conv3_grad.py and for the same reason: grad_y is multiplied by
(y_gpu > 0) and the linear layer is differentiated.  Errors are max-normalised per gradient tensor (update_cases.err);
the tolerances are the project's standing gradient tolerances: fp32 1e-5, fp16 5e-3, bf16 1e-2."""
from __future__ import annotations

import functools

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
FWD_TOL = {"fp32": 1e-5, "fp16": 1e-2, "bf16": 1e-2}   # the forward's tolerances (include/dvccorr.h, dvc_conv7_flow)
PRECISIONS = ("fp32", "fp16", "bf16")
BOUND = 1.0 / float(np.sqrt(3 * 343))


def _uniform(seed, shape, bound=1.0):
    return torch.from_numpy(prng.uniform(seed, tuple(shape), -bound, bound))


def _layer(seed, B, vol, cout=64):
    """flow, weight, bias, grad_y of a synthetic convf1, CPU float32."""
    return (_uniform(seed, (B, 3, *vol), 2.0), _uniform(seed + 1, (cout, 3, 7, 7, 7), BOUND),
            _uniform(seed + 2, (cout,), BOUND), _uniform(seed + 3, (B, cout, *vol)))


def _gpu(flow, w, b, gy, precision, need=(False, True, True)):
    """y and the gradients (dflow, dw, db) of conv7x7x7_flow_ad on the GPU; entries not asked for are None."""
    import dvccorr
    ts = [t.to(DEV).clone().requires_grad_(n) for t, n in zip((flow, w, b), need)]
    y = dvccorr.conv7x7x7_flow_ad(*ts, precision=precision)
    y.backward(gy.to(DEV))
    return (y.detach(),) + tuple(t.grad for t in ts)


def _ref(flow, w, b, g):
    """Gradients (dflow, dw, db) of the linear layer conv3d(flow, w, padding=3) + b for the output gradient g: float64
    on the CPU."""
    ts = [t.double().requires_grad_(True) for t in (flow, w, b)]
    F.conv3d(*ts, padding=3).backward(g.double())
    return tuple(t.grad for t in ts)


def _check(flow, w, b, gy, precision, what="", need=(False, True, True)):
    y, *got = _gpu(flow, w, b, gy, precision, need)
    g = gy * (y.cpu() > 0)
    errs = {n: uc.err(a, r) for n, a, r in zip(("dflow", "dw", "db"), got, _ref(flow, w, b, g)) if a is not None}
    print(what, precision, {k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) <= TOL[precision], (what, precision, errs)
    return y, got


# ---------------------------------------------------------------------------------------------------------------
# 1. the reference's own gradients (tests/golden/gen_update_block_grad_golden.py)
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture():
    """The fixture's inputs and, from float64 autograd of its loss on the CPU, the output gradient of convf1: flow,
    weight, bias, flo1 (float32 reference activation), g_out = d loss / d relu(convf1(flow)), and the stored arrays."""
    ref = {k: torch.from_numpy(v) for k, v in load_golden("updblk_grad_b2_597.npz").items()}
    s_net, s_delta, _, s_flow = (int(v) for v in ref["seeds"])
    p, c = uc.params("upd_b2_597"), uc.case("upd_b2_597")
    pd = {n: t.double() for n, t in p.items()}
    flow = torch.from_numpy(prng.uniform(s_flow, tuple(c["flow"].shape), -2.0, 2.0))
    with torch.no_grad():
        flo1_32 = F.relu(uc.rl._conv(p, "encoder.convf1", flow, 3))
    flo1 = F.relu(uc.rl._conv(pd, "encoder.convf1", flow.double(), 3)).detach().requires_grad_(True)
    flo2 = F.relu(uc.rl._conv(pd, "encoder.convf2", flo1, 1))
    mot = F.relu(uc.rl._conv(pd, "encoder.conv", torch.cat([c["cor"].double(), flo2], dim=1), 1))
    net = uc.rl.sep_gru(pd, c["net0"].double(), torch.cat([c["context"].double(), mot, flow.double()], dim=1))
    delta = uc.rl._conv(pd, "flow_head.conv2", F.relu(uc.rl._conv(pd, "flow_head.conv1", net, 1)), 1)
    loss = (_uniform(s_net, net.shape).double() * net).sum() + (_uniform(s_delta, delta.shape).double() * delta).sum()
    loss.backward()
    return flow, p["encoder.convf1.weight"], p["encoder.convf1.bias"], flo1_32, flo1.grad.float(), ref


@pytest.mark.parametrize("precision", PRECISIONS)
def test_reference_fixture(precision):
    """convf1's weight and bias gradients inside the reference's whole update block (case upd_b2_597 with the fixture's
    flow seed; all 343 taps see the volume), with the output gradient of convf1 taken from float64 autograd of the
    fixture's loss on the CPU.  The stored gradients carry the reference's mask [y_ref > 0], the op's carries
    [y_gpu > 0]: the reference under the op's mask is the stored one plus the linear layer's float64 gradients of
    g_out ([y_gpu > 0] - [y_ref > 0]) (the _mask_term rule of tests/test_gpu_conv3_grad.py); the masks may differ only
    where both activations are within the forward's tolerance of zero."""
    flow, w, b, y_ref, g_out, ref = _fixture()
    y, _, dw, db = _gpu(flow, w, b, g_out, precision)
    y = y.cpu()
    flip = (y_ref > 0) != (y > 0)
    lim = FWD_TOL[precision] * float(y_ref.abs().max())
    print(precision, "mask bits that differ:", int(flip.sum()), "of", flip.numel())
    assert not flip.any() or max(float(y_ref[flip].abs().max()), float(y[flip].abs().max())) <= lim
    _, m_dw, m_db = _ref(flow, w, b, g_out.double() * ((y > 0).double() - (y_ref > 0).double()))
    errs = {"convf1_dw": uc.err(dw, ref["convf1_dw"].double() + m_dw),
            "convf1_db": uc.err(db, ref["convf1_db"].double() + m_db)}
    print(precision, {k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) <= TOL[precision], errs


# ---------------------------------------------------------------------------------------------------------------
# 2. seams of the K-block and of the slabs
# ---------------------------------------------------------------------------------------------------------------
def _seam_volumes():
    from dvccorr import _lib
    ext = (_lib.CONV7_WGRAD_KH, _lib.CONV7_WGRAD_KW, _lib.CONV7_WGRAD_KD)
    vols = [(1, 1, 1), (2, 1, 5)]
    for axis in range(3):
        for n in (ext[axis] - 1, ext[axis], ext[axis] + 1, 2 * ext[axis] + 1):
            v = [3, 3, 3]
            v[axis] = n
            if tuple(v) not in vols:
                vols.append(tuple(v))
    return vols


@pytest.mark.parametrize("vol", _seam_volumes(), ids=lambda v: "x".join(map(str, v)))
def test_seams(vol):
    """Every gradient at the fp32 tolerance; a tap that no voxel of the volume sees gets an exact zero."""
    layer = _layer(9300, 1, vol)
    _, (_, dw, _) = _check(*layer, "fp32", f"seam {vol}")
    seen = [np.array([any(0 <= v + k - 3 < n for v in range(n)) for k in range(7)]) for n in vol]
    unseen = torch.from_numpy(~np.einsum("a,b,c->abc", *seen))
    if vol in ((1, 1, 1), (2, 1, 5)):
        assert int(unseen.sum()) == {(1, 1, 1): 342, (2, 1, 5): 343 - 3 * 1 * 7}[vol]
    assert not dw.cpu()[:, :, unseen].any()
    assert dw.cpu()[:, :, ~unseen].any()


def test_slab_seams():
    """One volume with fewer K-blocks than the slab rule would like, and one whose K-block count is no multiple of its
    slab count (the last slab is short)."""
    from dvccorr import _lib, ops
    want = -(-_lib.CONV7_WGRAD_TARGET // -(-65 // _lib.CONV7_WGRAD_TILES))
    nbox, per, nslab = ops.conv7_wgrad_slabs(1, 3, 5, 17)
    assert nbox == 4 < want and (per, nslab) == (1, 4)
    _check(*_layer(9310, 1, (3, 5, 17)), "fp32", "few blocks")
    vol = (3, 3, 23 * _lib.CONV7_WGRAD_KD - 5)
    nbox, per, nslab = ops.conv7_wgrad_slabs(1, *vol)
    assert nbox == 23 > want and per == 2 and nslab == 12 and nbox % nslab != 0
    _check(*_layer(9320, 1, vol), "fp32", "short last slab")


# ---------------------------------------------------------------------------------------------------------------
# 3. batch, 4. exact probes
# ---------------------------------------------------------------------------------------------------------------
def test_batch_of_two():
    """Batch elements sum into dW and db."""
    flow, w, b, gy = _layer(9400, 2, (5, 9, 7))
    for precision in PRECISIONS:
        _check(flow, w, b, gy, precision, "B=2")
    _, _, dw, db = _gpu(flow, w, b, gy, "fp32")
    parts = [_gpu(flow[i:i + 1], w, b, gy[i:i + 1], "fp32") for i in range(2)]
    assert uc.err(parts[0][2] + parts[1][2], dw) <= 1e-6 and uc.err(parts[0][3] + parts[1][3], db) <= 1e-6


@pytest.mark.parametrize("precision", PRECISIONS)
def test_exact_counts(precision):
    """flow = grad_y = 1 (weight 0, bias 1, so every output is alive): dW[o, ci, tap] counts the voxels whose tap lies
    inside the volume, db the voxel count.  Small integers: exact in every precision."""
    B, vol = 2, (3, 4, 18)
    _, _, dw, db = _gpu(torch.ones(B, 3, *vol), torch.zeros(64, 3, 7, 7, 7), torch.ones(64), torch.ones(B, 64, *vol),
                        precision)
    inside = [np.array([[0 <= v + k - 3 < n for v in range(n)] for k in range(7)]) for n in vol]   # [tap][voxel]
    taps = np.einsum("ah,bw,cd->abchwd", *inside).astype(np.float64).sum(axis=(3, 4, 5))
    assert torch.equal(dw.cpu().double(), torch.from_numpy(B * taps).expand(64, 3, 7, 7, 7))
    assert torch.equal(db.cpu(), torch.full((64,), float(B * np.prod(vol))))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_dead_relu_gives_zero_gradients(precision):
    flow, w, b, gy = _layer(9500, 1, (3, 4, 18))
    y, _, dw, db = _gpu(torch.zeros_like(flow), w, -b.abs() - 0.1, gy, precision)
    assert not y.any() and not dw.any() and not db.any()


# ---------------------------------------------------------------------------------------------------------------
# 5. determinism and linearity at the benchmark's size
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_deterministic_and_linear_at_bench_size(precision):
    """Two runs are bit-identical; for fp32 and bf16 (power-of-two scaling commutes with their roundings) grad_y 2^-20
    gives exactly 2^-20 x the gradients."""
    flow, w, b, gy = (t.to(DEV) for t in _layer(9600, 1, (32, 32, 32)))
    first = _gpu(flow, w, b, gy, precision)[2:]
    again = _gpu(flow, w, b, gy, precision)[2:]
    for a, c in zip(first, again):
        assert a.abs().max() > 0 and torch.equal(a, c)
    if precision != "fp16":
        small = _gpu(flow, w, b, gy * 2.0 ** -20, precision)[2:]
        for a, c in zip(first, small):
            assert torch.equal(a * 2.0 ** -20, c)


# ---------------------------------------------------------------------------------------------------------------
# 6. needs_input_grad subsets, no_grad, double backward, opcheck, the slow and the library paths
# ---------------------------------------------------------------------------------------------------------------
def test_needs_input_grad_subsets():
    import dvccorr
    layer = _layer(9700, 1, (4, 4, 4))
    full = _gpu(*layer, "fp32")
    _, df, dw, db = _gpu(*layer, "fp32", need=(False, True, False))
    assert df is None and db is None and torch.equal(dw, full[2])
    _, df, dw, db = _gpu(*layer, "fp32", need=(False, False, True))
    assert df is None and dw is None and torch.equal(db, full[3])
    flow, w, b, _ = (t.to(DEV) for t in layer)
    w, b = w.requires_grad_(True), b.requires_grad_(True)
    with torch.no_grad():
        assert not dvccorr.conv7x7x7_flow_ad(flow, w, b).requires_grad
    assert not dvccorr.conv7x7x7_flow_ad(flow, w.detach(), b.detach()).requires_grad
    y = dvccorr.conv7x7x7_flow_ad(flow, w, b)
    with pytest.raises(NotImplementedError, match="double backward"):
        torch.autograd.grad(y, w, torch.ones_like(y).requires_grad_(True), create_graph=True)


def test_opcheck():
    import dvccorr.library  # noqa: F401
    flow, w, b, gy = (t.to(DEV) for t in _layer(9800, 1, (4, 4, 4)))
    rg = lambda t: t.clone().requires_grad_(True)   # noqa: E731
    torch.library.opcheck(torch.ops.dvccorr.conv7_ad.default, (flow, rg(w), rg(b), 0))
    torch.library.opcheck(torch.ops.dvccorr.conv7_ad.default, (rg(flow), rg(w), b, 2))
    torch.library.opcheck(torch.ops.dvccorr.conv7_wgrad.default, (flow, gy, 0))
    torch.library.opcheck(torch.ops.dvccorr.conv7_wgrad.default, (flow, gy, 1))


def test_flow_that_requires_grad():
    """The slow path (torch.nn.grad.conv3d_input of the masked gradient in float32) against float64."""
    _check(*_layer(9900, 1, (4, 4, 4)), "fp32", "d flow", need=(True, True, True))


def test_fallback_outside_the_kernels_shapes():
    """A 7 x 7 x 7 layer with 32 outputs runs F.conv3d in float32, still differentiable."""
    _check(*_layer(9910, 1, (5, 4, 17), cout=32), "fp32", "3->32", need=(True, True, True))
