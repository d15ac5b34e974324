"""GPU: dvccorr.UpdateBlock / conv3x3x3 (k_conv3_mfma and k_conv7_flow, csrc/conv3.hip) against the reference's
BasicUpdateBlock fixtures (tests/golden/upd_*.npz) and the CPU checker (update_cases, pinned by test_update_cpu.py).

Tolerances (max-normalised): fp32 1e-5 (operands split into bf16 hi + lo), fp16 / bf16 1e-2 -- the project's standing
tolerances (tests/test_gpu_gru.py)."""
from __future__ import annotations

import pytest
import torch

import prng
import update_cases as uc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TOL = {"fp32": 1e-5, "fp16": 1e-2, "bf16": 1e-2}
PRECISIONS = ["fp32", "fp16", "bf16"]


def _dev(p):
    return {n: t.to(DEV) for n, t in p.items()}


def _uniform(seed, shape, b=1.0):
    return torch.from_numpy(prng.uniform(seed, tuple(shape), -b, b))


def _run_layer(layer, p_dev, srcs, precision):
    """One layer through the C entry point's Python wrapper, fed the given (device) inputs."""
    import dvccorr
    from dvccorr import ops
    w, b = p_dev[layer + ".weight"], p_dev[layer + ".bias"]
    relu = uc.LAYERS[layer][3]
    if layer == "encoder.convf1":
        dtype = ops.dtype_code(precision)
        dst = torch.empty((srcs[0].shape[0], 64) + tuple(srcs[0].shape[2:]), device=DEV)
        return ops.conv7_flow(srcs[0], ops.conv7_flow_pack(w, b, dtype), dst, dtype)
    return dvccorr.conv3x3x3(srcs[0], w, b, relu=relu, precision=precision, x2=srcs[1] if len(srcs) > 1 else None)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", uc.CASES)
def test_fixture_layers(name, precision):
    """Each layer from the reference's stored input activation against the reference's stored output."""
    pd, c = _dev(uc.params(name)), uc.case(name)
    errs = {}
    for layer in uc.layers_of(name):
        got = _run_layer(layer, pd, [t.to(DEV) for t in uc.layer_inputs(c, layer)], precision)
        ref = c[uc.LAYERS[layer][1]]
        assert got.dtype == torch.float32 and got.shape == ref.shape
        errs[layer] = uc.err(got, ref)
    print(name, precision, {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= TOL[precision], (name, precision, errs)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", uc.CASES)
def test_fixture_block(name, precision):
    import dvccorr
    pd, c = _dev(uc.params(name)), uc.case(name)
    blk = dvccorr.UpdateBlock(pd, precision=precision)
    net, delta, log_b = blk(c["net0"].to(DEV), c["context"].to(DEV), c["flow"].to(DEV), cor=c["cor"].to(DEV))
    errs = {"net": uc.err(net, c["net"]), "delta_flow": uc.err(delta, c["delta_flow"])}
    if "log_b" in c:
        assert log_b.shape == c["log_b"].shape and log_b.shape[1] == 4
        errs["log_b"] = uc.err(log_b, c["log_b"])
    else:
        assert log_b is None
    print(name, precision, {k: f"{v:.2e}" for k, v in errs.items()})
    assert net.dtype == delta.dtype == torch.float32
    assert max(errs.values()) <= TOL[precision], (name, precision, errs)


def test_raw_corr_slow_path():
    """corr instead of cor: the 1 x 1 x 1 convc1 runs in the library; same result as cor at the fp32 tolerance."""
    import dvccorr
    pd, c = _dev(uc.params("upd_215")), uc.case("upd_215")
    blk = dvccorr.UpdateBlock(pd, precision="fp32")
    net, delta, log_b = blk(c["net0"].to(DEV), c["context"].to(DEV), c["flow"].to(DEV), corr=c["corr"].to(DEV))
    e = max(uc.err(net, c["net"]), uc.err(delta, c["delta_flow"]), uc.err(log_b, c["log_b"]))
    print(f"raw corr: {e:.2e}")
    assert e <= TOL["fp32"]


def _seam_lengths(t):
    return [t - 1, t, t + 1, 2 * t + 1]


def _seam_cases():
    from dvccorr import _lib
    out = []
    for kernel, tiles in (("conv3", (_lib.CONV3_TH, _lib.CONV3_TW, _lib.CONV3_TD)),
                          ("conv7", (_lib.CONV7_TH, _lib.CONV7_TW, _lib.CONV7_TD))):
        for axis in range(3):
            for n in _seam_lengths(tiles[axis]):
                out.append(pytest.param(kernel, axis, n, id=f"{kernel}-axis{axis}-{n}"))
    return out


def _seam_params():
    p = uc.params()
    return p, _dev(p)


@pytest.fixture(scope="module")
def weights():
    return _seam_params()


@pytest.mark.parametrize("kernel,axis,n", _seam_cases())
def test_tile_seams(kernel, axis, n, weights):
    """An axis of T - 1, T, T + 1 and 2 T + 1 voxels (T the workgroup's box extent along it; the other two axes 3):
    the halo on both sides of a seam and the partial last box, at the fp32 tolerance against the CPU checker.
    conv3: encoder.conv (two sources, 128 -> 80, written into channels 64..143 of 147); conv7: encoder.convf1."""
    import dvccorr
    p, pd = weights
    vol = [3, 3]
    vol.insert(axis, n)
    if kernel == "conv3":
        cor = torch.relu(torch.from_numpy(prng.normal(8300 + axis, (1, 96, *vol))))
        flo = torch.relu(torch.from_numpy(prng.normal(8310 + axis, (1, 32, *vol))))
        with torch.no_grad():
            ref = uc.check_layer(p, "encoder.conv", cor, flo)
        out = torch.zeros((1, 147, *vol), device=DEV)
        dvccorr.conv3x3x3(cor.to(DEV), pd["encoder.conv.weight"], pd["encoder.conv.bias"], relu=True,
                          precision="fp32", x2=flo.to(DEV), out=out, out_offset=64)
        got = out[:, 64:144]
    else:
        flow = _uniform(8320 + axis, (1, 3, *vol), 2.0)
        with torch.no_grad():
            ref = uc.check_layer(p, "encoder.convf1", flow)
        got = _run_layer("encoder.convf1", pd, [flow.to(DEV)], "fp32")
    e = uc.err(got, ref)
    print(f"seam {kernel} axis {axis} length {n}: {e:.2e}")
    assert e <= TOL["fp32"], (kernel, axis, n, e)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_zero_padding_exact(precision):
    """All-ones input and weights, zero bias, no ReLU, on 4 x 5 x 6: every output is Cin x (in-volume taps of the
    voxel), exact in every precision.  Both kernels."""
    import dvccorr
    from dvccorr import ops
    vol = (4, 5, 6)

    def taps(k):
        one = torch.ones(1, 1, *vol)
        return torch.nn.functional.conv3d(one, torch.ones(1, 1, k, k, k), padding=k // 2)

    x = torch.ones(1, 40, *vol, device=DEV)
    got = dvccorr.conv3x3x3(x, torch.ones(24, 40, 3, 3, 3, device=DEV), torch.zeros(24, device=DEV),
                            precision=precision)
    assert torch.equal(got.cpu(), (40 * taps(3)).expand(1, 24, *vol))
    dtype = ops.dtype_code(precision)
    packed = ops.conv7_flow_pack(torch.ones(64, 3, 7, 7, 7, device=DEV), torch.zeros(64, device=DEV), dtype)
    # ReLU is part of the kernel; the sums are positive
    got7 = ops.conv7_flow(torch.ones(1, 3, *vol, device=DEV), packed, torch.empty(1, 64, *vol, device=DEV), dtype)
    assert torch.equal(got7.cpu(), (3 * taps(7)).expand(1, 64, *vol))


@pytest.mark.parametrize("cout,offset,total", [(80, 64, 147), (3, 5, 9)])
def test_slice_write(cout, offset, total):
    """The destination pre-filled with NaN: channels outside [offset, offset + cout) keep their bits (for cout = 3
    thirteen padded rows are never stored), and no NaN is inside the slice."""
    import dvccorr
    vol = (5, 6, 17)
    x = _uniform(8401, (2, 128, *vol)).to(DEV)
    w, b = _uniform(8402, (cout, 128, 3, 3, 3), 0.02), _uniform(8403, (cout,), 0.02)
    out = torch.full((2, total, *vol), float("nan"), device=DEV)
    bits = out.view(torch.int32).clone()
    dvccorr.conv3x3x3(x, w.to(DEV), b.to(DEV), precision="fp32", out=out, out_offset=offset)
    inside = out[:, offset:offset + cout]
    assert not torch.isnan(inside).any()
    keep = [i for i in range(total) if not offset <= i < offset + cout]
    assert torch.equal(out.view(torch.int32)[:, keep], bits[:, keep])
    with torch.no_grad():
        ref = uc.conv_ref(x.cpu(), w, b)
    assert uc.err(inside, ref) <= TOL["fp32"]


@pytest.mark.parametrize("c0,c1", [(96, 32), (40, 19)])
def test_channel_padding(c0, c1):
    """96 + 32 (full chunks) and 40 + 19 (a chunk that straddles the two sources, the last one partly empty) at fp32
    against the checker; 21 output channels (two tiles, the second partly empty)."""
    import dvccorr
    vol = (5, 4, 9)
    x0, x1 = _uniform(8501, (1, c0, *vol)), _uniform(8502, (1, c1, *vol))
    w, b = _uniform(8503, (21, c0 + c1, 3, 3, 3), 0.03), _uniform(8504, (21,), 0.03)
    with torch.no_grad():
        ref = uc.conv_ref(x0, w, b, relu=True, x2=x1)
    got = dvccorr.conv3x3x3(x0.to(DEV), w.to(DEV), b.to(DEV), relu=True, precision="fp32", x2=x1.to(DEV))
    e = uc.err(got, ref)
    print(f"channels {c0} + {c1}: {e:.2e}")
    assert e <= TOL["fp32"]


def _block_inputs(name):
    c = uc.case(name)
    return [c[k].to(DEV) for k in ("net0", "context", "flow", "cor")]


def test_determinism_input_safety_and_repack():
    import dvccorr
    pd = {n: t.clone() for n, t in _dev(uc.params("upd_215")).items()}
    net, ctx, flow, cor = _block_inputs("upd_215")
    keep = [t.clone() for t in (net, ctx, flow, cor)]
    blk = dvccorr.UpdateBlock(pd, precision="fp32")
    a, b = blk(net, ctx, flow, cor=cor), blk(net, ctx, flow, cor=cor)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert all(torch.equal(u, v) for u, v in zip((net, ctx, flow, cor), keep))
    pd["flow_head.conv2.weight"].mul_(2)                               # in-place update: re-pack
    c = blk(net, ctx, flow, cor=cor)
    assert torch.equal(c[0], a[0]) and not torch.equal(c[1], a[1]) and torch.equal(c[2], a[2])
    pd["encoder.convf1.weight"] = pd["encoder.convf1.weight"] * 2      # replaced tensor: re-pack
    d = blk(net, ctx, flow, cor=cor)
    assert not torch.equal(d[0], c[0])
    fresh = dvccorr.UpdateBlock(pd, precision="fp32")(net, ctx, flow, cor=cor)
    assert all(torch.equal(u, v) for u, v in zip(d, fresh))
    ctx.mul_(0.5)                                                      # changed context: copied again
    e = blk(net, ctx, flow, cor=cor)
    assert not torch.equal(e[0], d[0])
    fresh = dvccorr.UpdateBlock(pd, precision="fp32")(net, ctx, flow, cor=cor)
    assert all(torch.equal(u, v) for u, v in zip(e, fresh))
    ctx2 = ctx * 2                                                     # another context tensor
    f = blk(net, ctx2, flow, cor=cor)
    assert all(torch.equal(u, v) for u, v in zip(f, d))


def test_graph_capture():
    """One refinement iteration -- CorrBlock.lookup_convc1 -> UpdateBlock -> flow_step -- captured on one stream
    after a warm-up; replays equal eager bit for bit for two different coords1."""
    import dvccorr
    pd = _dev(uc.params())
    B, vol, T = 1, (8, 8, 8), (16, 16, 16)
    f0 = torch.from_numpy(prng.normal(8601, (B, 32, *vol))).to(DEV)
    f1 = torch.from_numpy(prng.normal(8602, (B, 32, *vol))).to(DEV)
    corr_fn = dvccorr.CorrBlock(f0, f1, 4, 4, precision="fp32")
    coords0 = dvccorr.coords_grid_3d(B, *vol, DEV)
    net, ctx, _, _ = _block_inputs("upd_888")
    blk = dvccorr.UpdateBlock(pd, precision="fp32")
    cw, cb = pd["encoder.convc1.weight"], pd["encoder.convc1.bias"]

    def iteration(coords1):
        cor = corr_fn.lookup_convc1(coords1, cw, cb)
        n, delta, _ = blk(net, ctx, coords1 - coords0, cor=cor)
        new, up = dvccorr.flow_step(coords1, delta, T)
        return n, new, up

    starts = [coords0 + torch.from_numpy(prng.uniform(8610 + i, (B, 3, *vol), -1.5, 1.5)).to(DEV) for i in range(2)]
    with torch.no_grad():
        eager = [[t.clone() for t in iteration(s)] for s in starts]       # also the warm-up
        static = starts[0].clone()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                outs = iteration(static)
        for start, want in zip(starts, eager):
            static.copy_(start)
            g.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(u, v) for u, v in zip(outs, want))


def test_fallback_composition(monkeypatch):
    """With the kernels' coverage predicates refusing every layer, the block runs the library composition and makes no
    kernel call; it equals the checker at the fp32 tolerance."""
    import dvccorr
    from dvccorr import ops, update
    p = uc.params("upd_215")
    c = uc.case("upd_215")

    def no_kernel(*a, **k):
        raise AssertionError("kernel path taken although the layer is refused")
    monkeypatch.setattr(update, "kernel_covers", lambda hidden, inp: False)
    monkeypatch.setattr(update, "conv_covers", lambda cin, cout: False)
    for fn in ("conv3", "conv3_pack", "conv7_flow", "conv7_flow_pack", "sep_gru", "gru_pack"):
        monkeypatch.setattr(ops, fn, no_kernel)
    got = dvccorr.UpdateBlock(_dev(p))(*_block_inputs("upd_215")[:3], cor=c["cor"].to(DEV))
    with torch.no_grad():
        ref = uc.checker(p, c["net0"], c["context"], c["flow"], cor=c["cor"])
    e = max(uc.err(a, r) for a, r in zip(got, ref))
    print(f"fallback: {e:.2e}")
    assert e <= TOL["fp32"]


def test_non_separable_gru_state_dict():
    """A ConvGRU3D state dict (gru.convz.weight): the GRU runs as the library composition, the other layers on the
    kernels."""
    import dvccorr
    p = {n: t for n, t in uc.params().items() if not n.startswith("gru.")}
    for i, g in enumerate("zrq"):
        p[f"gru.conv{g}.weight"] = _uniform(8701 + 2 * i, (96, 243, 3, 3, 3), 0.012)
        p[f"gru.conv{g}.bias"] = _uniform(8702 + 2 * i, (96,), 0.012)
    c = uc.case("upd_215")
    got = dvccorr.UpdateBlock(_dev(p), precision="fp32")(*_block_inputs("upd_215")[:3], cor=c["cor"].to(DEV))
    import torch.nn.functional as F
    with torch.no_grad():
        inp = torch.cat([c["context"], uc.rl.motion_features(p, c["flow"], cor=c["cor"])], dim=1)
        h = c["net0"]
        hx = torch.cat([h, inp], dim=1)
        z = torch.sigmoid(uc.rl._conv(p, "gru.convz", hx, 1))
        r = torch.sigmoid(uc.rl._conv(p, "gru.convr", hx, 1))
        q = torch.tanh(uc.rl._conv(p, "gru.convq", torch.cat([r * h, inp], dim=1), 1))
        net = (1 - z) * h + z * q
        delta = uc.rl._conv(p, "flow_head.conv2", F.relu(uc.rl._conv(p, "flow_head.conv1", net, 1)), 1)
    assert got[2] is None
    assert max(uc.err(got[0], net), uc.err(got[1], delta)) <= TOL["fp32"]


def test_opcheck():
    from dvccorr import ops
    import dvccorr.library  # noqa: F401
    vol = (4, 4, 4)
    x0 = _uniform(8801, (1, 40, *vol)).to(DEV)
    x1 = _uniform(8802, (1, 19, *vol)).to(DEV)
    w, b = _uniform(8803, (21, 59, 3, 3, 3), 0.03).to(DEV), _uniform(8804, (21,), 0.03).to(DEV)
    dst = torch.zeros(1, 30, *vol, device=DEV)
    torch.library.opcheck(torch.ops.dvccorr.conv3.default, (x0, x1, ops.conv3_pack(w, b, 0), dst, 4, 21, True, 0))
    torch.library.opcheck(torch.ops.dvccorr.conv3.default, (x0, None, ops.conv3_pack(w[:, :40].contiguous(), b, 2),
                                                            dst, 0, 21, False, 2))
    flow = _uniform(8805, (1, 3, *vol), 2.0).to(DEV)
    w7, b7 = _uniform(8806, (64, 3, 7, 7, 7), 0.03).to(DEV), _uniform(8807, (64,), 0.03).to(DEV)
    dst7 = torch.zeros(1, 64, *vol, device=DEV)
    torch.library.opcheck(torch.ops.dvccorr.conv7_flow.default, (flow, ops.conv7_flow_pack(w7, b7, 0), dst7, 0))


def test_grad_required_inputs_raise():
    import dvccorr
    pd = _dev(uc.params())
    net, ctx, flow, cor = _block_inputs("upd_215")
    blk = dvccorr.UpdateBlock(pd)
    for i in range(4):
        args = [net, ctx, flow, cor]
        args[i] = args[i].clone().requires_grad_(True)
        with pytest.raises(NotImplementedError):
            blk(*args[:3], cor=args[3])
    pg = dict(pd)
    pg["flow_head.conv1.bias"] = pd["flow_head.conv1.bias"].clone().requires_grad_(True)
    with pytest.raises(NotImplementedError):
        dvccorr.UpdateBlock(pg)(net, ctx, flow, cor=cor)
    with pytest.raises(NotImplementedError):
        dvccorr.conv3x3x3(net, pg["flow_head.conv1.weight"], pg["flow_head.conv1.bias"])
    with torch.no_grad():                                     # grad disabled: runs
        out = dvccorr.UpdateBlock(pg)(net, ctx, flow, cor=cor)
        assert not out[0].requires_grad and not out[1].requires_grad
