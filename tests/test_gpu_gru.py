"""GPU: dvccorr.sep_conv_gru / SepConvGRU (k_sep_gru_pass, csrc/gru.hip) against the reference's SepConvGRU3D
fixtures (tests/golden/gru_*.npz) and the CPU checker (raftdvc_loop.sep_gru, pinned by test_gru_cpu.py).

Tolerances (max-normalised): fp32 1e-5 (operands split into bf16 hi + lo), fp16 / bf16 1e-2 -- the project's standing
tolerances."""
from __future__ import annotations

import pytest
import torch

import gru_cases as gc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TOL = {"fp32": 1e-5, "fp16": 1e-2, "bf16": 1e-2}


def _dev(p):
    return {n: t.to(DEV) for n, t in p.items()}


@pytest.fixture(scope="module")
def weights():
    p = gc.params()
    return p, _dev(p)


def _passes(h, x, p_dev, precision):
    """h after each pass through the C entry point, as ops.sep_gru chains them."""
    from dvccorr import ops
    dtype = ops.dtype_code(precision)
    packed = ops.gru_pack(p_dev, dtype)
    out, cur = [], h.contiguous()
    for a in range(3):
        nxt = torch.empty_like(cur)
        ops.sep_gru_pass(cur, x, packed[a], nxt, a, dtype)
        out.append(nxt)
        cur = nxt
    return out


@pytest.mark.parametrize("precision", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("name", gc.CASES)
def test_fixture_passes(name, precision, weights):
    import dvccorr
    _, pd = weights
    h, x, ref = gc.inputs(name)
    hd, xd = h.to(DEV), x.to(DEV)
    got = _passes(hd, xd, pd, precision)
    end = dvccorr.sep_conv_gru(hd, xd, pd, precision=precision)
    errs = [gc.err(a, r) for a, r in zip(got, ref)] + [gc.err(end, ref[2])]
    print(f"{name} {precision}: after h {errs[0]:.2e}, w {errs[1]:.2e}, d {errs[2]:.2e}, end to end {errs[3]:.2e}")
    assert end.dtype == torch.float32 and end.shape == h.shape
    assert max(errs) <= TOL[precision], (name, precision, errs)


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("length", ["seg+1", "2seg+3"])
def test_segment_seams(axis, length, weights):
    """A conv axis of GRU_SEG + 1 and of 2 GRU_SEG + 3 voxels (the other two 3 and 4): the halo of r (S + 4), of the
    inputs (S + 8) and the zero r * h outside the volume, at the fp32 tolerance against the CPU checker."""
    import dvccorr
    from dvccorr import _lib
    p, pd = weights
    n = _lib.GRU_SEG + 1 if length == "seg+1" else 2 * _lib.GRU_SEG + 3
    vol = [3, 4]
    vol.insert(axis, n)
    import prng
    h = torch.from_numpy(prng.uniform(7600 + axis, (1, 96, *vol), -1.0, 1.0))
    x = torch.from_numpy(prng.normal(7610 + axis, (1, 147, *vol)))
    with torch.no_grad():
        ref = gc.checker(p, h, x)
    got = dvccorr.sep_conv_gru(h.to(DEV), x.to(DEV), pd, precision="fp32")
    e = gc.err(got, ref)
    print(f"seam axis {axis} length {n}: {e:.2e}")
    assert e <= TOL["fp32"], (axis, n, e)


def test_zero_padding_probe():
    """h = 1, x = 0 and weights that are nonzero on the two outermost taps only: every border voxel sees the
    zero padding of cat[h, x] and of cat[r * h, x]; the result equals the CPU checker at every border voxel."""
    import dvccorr
    p = gc.params(seed0=7700)
    for n, t in p.items():
        if n.endswith("weight"):
            a = 2 + "hwd".index(n.split(".")[0][-1])
            t.narrow(a, 1, 3).zero_()
    vol = (11, 6, 9)
    h, x = torch.ones(1, 96, *vol), torch.zeros(1, 147, *vol)
    with torch.no_grad():
        ref = gc.checker(p, h, x)
    got = dvccorr.sep_conv_gru(h.to(DEV), x.to(DEV), _dev(p), precision="fp32").cpu()
    border = torch.ones(vol, dtype=torch.bool)
    border[2:-2, 2:-2, 2:-2] = False
    d = ((got - ref).abs() / ref.abs().max())[:, :, border]
    print(f"zero-padding probe: border {float(d.max()):.2e}")
    assert float(d.max()) <= TOL["fp32"]
    inner = ref[0, :, 5, 3, 4]
    assert float((ref[0, :, 0, 0, 0] - inner).abs().max()) > 1e-3     # the probe does see the padding


def test_determinism_input_safety_and_repack(weights):
    import dvccorr
    _, pd = weights
    h, x, _ = gc.inputs("gru_b2_597")
    hd, xd = h.to(DEV), x.to(DEV)
    h0, x0 = hd.clone(), xd.clone()
    pd = {n: t.clone() for n, t in pd.items()}
    gru = dvccorr.SepConvGRU(pd, precision="fp32")
    a, b = gru(hd, xd), gru(hd, xd)
    assert torch.equal(a, b)
    assert torch.equal(hd, h0) and torch.equal(xd, x0)
    assert gru.packed(0) is gru.packed(0)                    # cached while the weights stand
    for n in pd:
        if n.endswith("weight"):
            pd[n].mul_(2)
    c = gru(hd, xd)
    assert not torch.equal(a, c)
    assert torch.equal(c, dvccorr.sep_conv_gru(hd, xd, pd, precision="fp32"))


def test_graph_capture(weights):
    """Three passes captured on one stream replay to the eager result bit for bit."""
    from dvccorr import ops
    _, pd = weights
    h, x, _ = gc.inputs("gru_888")
    hd, xd = h.to(DEV), x.to(DEV)
    packed = ops.gru_pack(pd, 0)
    eager = ops.sep_gru(hd, xd, packed, 0)
    a, b = torch.empty_like(hd), torch.empty_like(hd)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ops.sep_gru_pass(hd, xd, packed[0], a, 0, 0)
            ops.sep_gru_pass(a, xd, packed[1], b, 1, 0)
            ops.sep_gru_pass(b, xd, packed[2], a, 2, 0)
    a.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(a, eager)


def test_fallback_composition(monkeypatch):
    """Hidden 32, input 19: outside the kernel's shapes, so the F.conv3d composition runs and no kernel call is made."""
    import dvccorr
    from dvccorr import ops
    p = gc.params(32, 19)
    import prng
    h = torch.from_numpy(prng.uniform(7801, (1, 32, 4, 4, 4), -1.0, 1.0))
    x = torch.from_numpy(prng.normal(7802, (1, 19, 4, 4, 4)))

    def no_kernel(*a, **k):
        raise AssertionError("kernel path taken for an unsupported shape")
    monkeypatch.setattr(ops, "sep_gru", no_kernel)
    monkeypatch.setattr(ops, "sep_gru_pass", no_kernel)
    monkeypatch.setattr(ops, "gru_pack", no_kernel)
    got = dvccorr.sep_conv_gru(h.to(DEV), x.to(DEV), _dev(p))
    with torch.no_grad():
        ref = gc.checker(p, h, x)
    assert gc.err(got, ref) <= TOL["fp32"]


def test_opcheck(weights):
    from dvccorr import ops
    import dvccorr.library  # noqa: F401
    _, pd = weights
    import prng
    h = torch.from_numpy(prng.uniform(7901, (1, 96, 4, 4, 4), -1.0, 1.0)).to(DEV)
    x = torch.from_numpy(prng.normal(7902, (1, 147, 4, 4, 4))).to(DEV)
    torch.library.opcheck(torch.ops.dvccorr.sep_gru.default, (h, x, ops.gru_pack(pd, 0), 0))


def test_grad_required_inputs_raise(weights):
    import dvccorr
    _, pd = weights
    h = torch.zeros(1, 96, 4, 4, 4, device=DEV)
    x = torch.zeros(1, 147, 4, 4, 4, device=DEV)
    with pytest.raises(NotImplementedError):
        dvccorr.sep_conv_gru(h.clone().requires_grad_(True), x, pd)
    with pytest.raises(NotImplementedError):
        dvccorr.sep_conv_gru(h, x.clone().requires_grad_(True), pd)
    pg = dict(pd)
    pg["convr_w.bias"] = pd["convr_w.bias"].clone().requires_grad_(True)
    with pytest.raises(NotImplementedError):
        dvccorr.SepConvGRU(pg)(h, x)
    with torch.no_grad():                                     # grad disabled: runs
        assert dvccorr.SepConvGRU(pg)(h, x).requires_grad is False
