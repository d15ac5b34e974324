"""GPU: dvccorr.sep_conv_gru_ad -- the backward of the fused SepConvGRU3D (csrc/gru_grad.hip).

The reference is float64 CPU autograd through gru_cases._one_pass / gru_cases.checker on the same inputs (and the
reference's own autograd in grugrad_215.npz); errors are max-normalised per gradient tensor (gru_cases.err);
tolerances are the project's standing gradient tolerances.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import gru_cases
import prng
from conftest import load_golden

pytestmark = pytest.mark.gpu

PRECISIONS = ("fp32", "fp16", "bf16")
TOL = {"fp32": 1e-5, "fp16": 5e-3, "bf16": 1e-2}
DEV = "cuda:0"
SEG = 8   # DVC_GRU_SEG


def _uniform(seed, shape, bound=1.0):
    return torch.from_numpy(prng.uniform(seed, tuple(shape), -bound, bound))


def _case(seed, inp, B, vol, hidden=96):
    h = _uniform(seed, (B, hidden) + tuple(vol))
    x = torch.from_numpy(prng.normal(seed + 1, (B, inp) + tuple(vol)))
    c = _uniform(seed + 2, (B, hidden) + tuple(vol))
    return h, x, c


def _ref(p, h, x, c):
    """float64 autograd of sum(c * gru(h, x)): {'h': .., 'x': .., '<weight name>': ..}"""
    pd = {n: t.double().requires_grad_(True) for n, t in p.items()}
    hd, xd = h.double().requires_grad_(True), x.double().requires_grad_(True)
    (c.double() * gru_cases.checker(pd, hd, xd)).sum().backward()
    return {"h": hd.grad, "x": xd.grad, **{n: t.grad for n, t in pd.items()}}


def _gpu(p, h, x, c, precision, need=None):
    """The same gradients from dvccorr.sep_conv_gru_ad; need: the names that require grad (default: all)."""
    import dvccorr
    names = ("h", "x") + tuple(p) if need is None else tuple(need)
    pg = {n: t.to(DEV).requires_grad_(n in names) for n, t in p.items()}
    hg, xg = h.to(DEV).requires_grad_("h" in names), x.to(DEV).requires_grad_("x" in names)
    out = dvccorr.sep_conv_gru_ad(hg, xg, pg, precision=precision)
    (c.to(DEV) * out).sum().backward()
    return {"h": hg.grad, "x": xg.grad, **{n: t.grad for n, t in pg.items()}}, out.detach()


def _compare(got, ref, precision, what, names=None):
    errs = {n: gru_cases.err(got[n], ref[n]) for n in (names or ref)}
    worst = max(errs, key=errs.get)
    print(f"{what} {precision}: worst {worst} {errs[worst]:.3e}")
    assert errs[worst] < TOL[precision], (what, precision, worst, errs[worst])


# 1. the reference's own autograd -----------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_reference_fixture(precision):
    g = load_golden("grugrad_215.npz")
    p = gru_cases.params()
    h, x, _ = gru_cases.inputs("gru_215")
    c = _uniform(int(np.asarray(g["seed"]).reshape(-1)[0]), h.shape)
    got, _ = _gpu(p, h, x, c, precision)
    ref = {"h": torch.from_numpy(g["d_h"]), "x": torch.from_numpy(g["d_x"])}
    for n in p:
        if n.endswith(".bias"):
            ref[n] = torch.from_numpy(g[n])
        else:
            ref[n] = torch.from_numpy(g[n + "8"])
            got[n] = got[n][::8]
    _compare(got, ref, precision, "fixture")


# 2. one pass through the C-level wrappers ---------------------------------------------------------------------------
def _one_pass_gpu(p, h, x, c, a, precision):
    from dvccorr import ops
    dt = ops.dtype_code(precision)
    pg = {n: t.to(DEV) for n, t in p.items()}
    hg, xg, cg = h.to(DEV), x.to(DEV), c.to(DEV)
    save, out = torch.empty((3,) + tuple(h.shape), device=DEV), torch.empty_like(hg)
    ops.sep_gru_pass_save(hg, xg, ops.gru_pack(pg, dt)[a], out, save, a, dt)
    z, r, q = save[0], save[1], save[2]
    aq, az, dh, dbq, dbz = ops.gru_grad_prep(cg, z, q, hg)
    dx = torch.empty_like(xg)
    ar, dbr = ops.sep_gru_dgrad(aq, az, hg, r, ops.gru_pack_dgrad(pg, dt)[a], dh, dx, a, False, dt)
    dw = ops.gru_wgrad(hg, xg, r, az, ar, aq, a, dt)
    ax = gru_cases.AXES[a]
    got = {"h": dh, "x": dx}
    for k, (gate, db) in enumerate(zip("zrq", (dbz, dbr, dbq))):
        got[f"conv{gate}_{ax}.weight"] = dw[k].reshape(p[f"conv{gate}_{ax}.weight"].shape)
        got[f"conv{gate}_{ax}.bias"] = db
    return got, out


def _one_pass_ref(p, h, x, c, a):
    ax = gru_cases.AXES[a]
    one = {f"gru.conv{g}_{ax}.{k}": p[f"conv{g}_{ax}.{k}"].double().requires_grad_(True)
           for g in "zrq" for k in ("weight", "bias")}
    hd, xd = h.double().requires_grad_(True), x.double().requires_grad_(True)
    out = gru_cases._one_pass(one, hd, xd, ax)
    (c.double() * out).sum().backward()
    return {"h": hd.grad, "x": xd.grad, **{n[4:]: t.grad for n, t in one.items()}}, out.detach()


def _pass_volume(a, length, others):
    vol = list(others)
    vol.insert(a, length)
    return tuple(vol)


_PASS_CASES = [(a, length, others, "fp32") for a in range(3) for length in (1, SEG, SEG + 1, 2 * SEG + 3)
               for others in ((3, 4), (17, 1))]
_PASS_CASES += [(0, SEG + 1, (3, 4), "fp16"), (1, 2 * SEG + 3, (3, 4), "bf16"), (2, SEG + 1, (17, 1), "fp16"),
                (2, 2 * SEG + 3, (3, 4), "bf16"), (1, SEG, (17, 1), "fp16"), (0, 2 * SEG + 3, (17, 1), "bf16")]


@pytest.mark.parametrize("a,length,others,precision", _PASS_CASES,
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_single_pass(a, length, others, precision):
    vol = _pass_volume(a, length, others)
    p = gru_cases.params()
    h, x, c = _case(9100 + 10 * a + length, 147, 1, vol)
    got, out = _one_pass_gpu(p, h, x, c, a, precision)
    ref, out_ref = _one_pass_ref(p, h, x, c, a)
    assert gru_cases.err(out, out_ref) < (1e-5 if precision == "fp32" else 1e-2)
    _compare(got, ref, precision, f"pass {gru_cases.AXES[a]} {vol}")


# 3. input channel counts -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("inp", (147, 160, 33, 1))
def test_input_channel_counts(inp, precision):
    p = gru_cases.params(96, inp, seed0=None if inp == 147 else 7600 + inp)
    h, x, c = _case(9200 + inp, inp, 1, (5, 4, 9))
    got, _ = _gpu(p, h, x, c, precision)
    _compare(got, _ref(p, h, x, c), precision, f"input {inp}")


# 4. batch of two ---------------------------------------------------------------------------------------------------
def test_batch_of_two():
    p = gru_cases.params()
    h, x, c = _case(9300, 147, 2, (5, 9, 7))
    got, _ = _gpu(p, h, x, c, "fp32")
    _compare(got, _ref(p, h, x, c), "fp32", "batch of two")
    c0 = c.clone()
    c0[1] = 0
    got0, _ = _gpu(p, h, x, c0, "fp32")
    assert not got0["h"][1].any() and not got0["x"][1].any()
    alone, _ = _gpu(p, h[:1], x[:1], c[:1], "fp32")
    for n in p:   # element 1 adds exact zeros to every sum
        assert torch.equal(got0[n], alone[n]), n
    assert torch.equal(got0["h"][0], alone["h"][0]) and torch.equal(got0["x"][0], alone["x"][0])


# 5. locality probes (exact) ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_zero_gradient_gives_zero(precision):
    p = gru_cases.params()
    h, x, c = _case(9400, 147, 1, (5, 4, 9))
    got, _ = _gpu(p, h, x, torch.zeros_like(c), precision)
    for n, t in got.items():
        assert not t.any(), n


@pytest.mark.parametrize("a", range(3))
def test_single_voxel_stays_in_its_line(a):
    p = gru_cases.params()
    length = 2 * SEG + 3
    vol = _pass_volume(a, length, (3, 4))
    h, x, _ = _case(9500 + a, 147, 1, vol)
    for pos in (0, length // 2, length - 1):
        where = [1, 2]
        where.insert(a, pos)
        c = torch.zeros_like(h)
        c[0, 5, where[0], where[1], where[2]] = 1.0
        c[0, 90, where[0], where[1], where[2]] = -0.5
        got, _ = _one_pass_gpu(p, h, x, c, a, "fp32")
        for n in ("h", "x"):
            g = got[n].cpu().movedim(2 + a, -1)            # (1, C, other0, other1, length)
            line = g[:, :, 1, 2].clone()
            assert line.any(), (n, pos)
            g[:, :, 1, 2] = 0
            assert not g.any(), (n, pos, "another line")
            far = [i for i in range(length) if abs(i - pos) > 4]
            assert not line[..., far].any(), (n, pos, "beyond +-4")


# 6. the forward is sep_conv_gru's ----------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_forward_identity(precision):
    import dvccorr
    p = gru_cases.params()
    h, x, c = _case(9600, 147, 2, (5, 9, 7))
    pg = {n: t.to(DEV) for n, t in p.items()}
    with torch.no_grad():
        plain = dvccorr.sep_conv_gru(h.to(DEV), x.to(DEV), pg, precision=precision)
        ad = dvccorr.sep_conv_gru_ad(h.to(DEV), x.to(DEV), pg, precision=precision)
        assert not ad.requires_grad
    _, trained = _gpu(p, h, x, c, precision)
    assert torch.equal(plain, ad) and torch.equal(plain, trained)


# 7. determinism at the benchmark's size ----------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_deterministic_and_linear_at_bench_size(precision):
    p = gru_cases.params()
    h, x, c = _case(9700, 147, 1, (32, 32, 32))
    first, _ = _gpu(p, h, x, c, precision)
    second, _ = _gpu(p, h, x, c, precision)
    for n in first:
        assert torch.equal(first[n], second[n]), n
        assert torch.isfinite(first[n]).all(), n
    if precision != "fp16":   # fp16 operands leave its range under the scaling
        scaled, _ = _gpu(p, h, x, c * 2.0 ** -20, precision)
        for n in first:
            assert torch.equal(scaled[n], first[n] * 2.0 ** -20), n


# 8. needs_input_grad subsets ---------------------------------------------------------------------------------------
def test_needs_input_grad_subsets():
    import dvccorr
    p = gru_cases.params()
    h, x, c = _case(9800, 147, 1, (5, 4, 9))
    full, _ = _gpu(p, h, x, c, "fp32")
    for need in (("h",), ("x",), ("convr_w.bias",), ("convq_d.weight", "x")):
        got, _ = _gpu(p, h, x, c, "fp32", need=need)
        for n in full:
            if n in need:
                assert torch.equal(got[n], full[n]), (need, n)
            else:
                assert got[n] is None, (need, n)
    pg = {n: t.to(DEV).requires_grad_(True) for n, t in p.items()}
    with torch.no_grad():
        assert not dvccorr.sep_conv_gru_ad(h.to(DEV), x.to(DEV), pg).requires_grad
    hg = h.to(DEV).requires_grad_(True)
    out = dvccorr.sep_conv_gru_ad(hg, x.to(DEV), pg, precision="fp32")
    gy = c.to(DEV).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="double backward"):
        torch.autograd.grad(out, hg, gy, create_graph=True)


# 9. opcheck --------------------------------------------------------------------------------------------------------
def test_opcheck():
    import dvccorr
    import dvccorr.library  # noqa: F401
    from dvccorr import ops
    p = gru_cases.params()
    h, x, c = (t.to(DEV) for t in _case(9900, 147, 1, (3, 4, 9)))
    ws = [p[n].to(DEV) for n in dvccorr.update.GRU_WEIGHT_NAMES]
    rg = lambda t: t.clone().requires_grad_(True)   # noqa: E731
    torch.library.opcheck(torch.ops.dvccorr.sep_gru_ad.default, (rg(h), rg(x), [rg(w) for w in ws], 0))
    torch.library.opcheck(torch.ops.dvccorr.sep_gru_ad.default, (rg(h), x, ws, 2))
    torch.library.opcheck(torch.ops.dvccorr.gru_pack_dgrad.default, (ws, 0))
    _, saved = torch.ops.dvccorr.sep_gru_ad(h, x, ws, 0)
    z, r, q = saved[6], saved[7], saved[8]
    torch.library.opcheck(torch.ops.dvccorr.gru_grad_prep.default, (c, z, q, saved[10]))
    aq, az, dh, _, _ = ops.gru_grad_prep(c, z, q, saved[10])
    packed = torch.ops.dvccorr.gru_pack_dgrad(ws, 1)
    torch.library.opcheck(torch.ops.dvccorr.gru_dgrad.default,
                          (aq, az, saved[10], r, packed, dh.clone(), torch.zeros_like(x), 2, True, 1))
    torch.library.opcheck(torch.ops.dvccorr.gru_dgrad.default, (aq, az, saved[10], r, packed, dh.clone(), None, 2, False, 1))
    ar, _ = ops.sep_gru_dgrad(aq, az, saved[10], r, packed[2], dh, None, 2, False, 1)
    torch.library.opcheck(torch.ops.dvccorr.gru_wgrad.default, (saved[10], x, r, az, ar, aq, 2, 0))


# 10. a chain with the differentiable 3 x 3 x 3 layers ----------------------------------------------------------------
def test_chain_with_conv3_ad():
    import dvccorr
    import torch.nn.functional as F
    p = gru_cases.params()
    h, x, _ = _case(10000, 147, 1, (3, 4, 9))
    w1, b1 = _uniform(10010, (128, 96, 3, 3, 3), 0.02), _uniform(10011, (128,), 0.02)
    w2, b2 = _uniform(10012, (3, 128, 3, 3, 3), 0.02), _uniform(10013, (3,), 0.02)
    c = _uniform(10014, (1, 3, 3, 4, 9))
    name = "convq_w.weight"
    pg = {n: t.to(DEV).requires_grad_(n == name) for n, t in p.items()}
    hg, xg = h.to(DEV).requires_grad_(True), x.to(DEV).requires_grad_(True)
    net = dvccorr.sep_conv_gru_ad(hg, xg, pg, precision="fp32")
    hid = dvccorr.conv3x3x3_ad(net, w1.to(DEV), b1.to(DEV), relu=True, precision="fp32")
    (c.to(DEV) * dvccorr.conv3x3x3_ad(hid, w2.to(DEV), b2.to(DEV), precision="fp32")).sum().backward()
    pd = {n: t.double().requires_grad_(n == name) for n, t in p.items()}
    hd, xd = h.double().requires_grad_(True), x.double().requires_grad_(True)
    hid_d = F.relu(F.conv3d(gru_cases.checker(pd, hd, xd), w1.double(), b1.double(), padding=1))
    (c.double() * F.conv3d(hid_d, w2.double(), b2.double(), padding=1)).sum().backward()
    _compare({"h": hg.grad, "x": xg.grad, name: pg[name].grad}, {"h": hd.grad, "x": xd.grad, name: pd[name].grad},
             "fp32", "chain")


# 11. outside the kernels' shapes ------------------------------------------------------------------------------------
def test_fallback_outside_the_kernels_shapes():
    p = gru_cases.params(32, 19, seed0=7700)
    h, x, c = _case(10100, 19, 1, (3, 4, 5), hidden=32)
    got, _ = _gpu(p, h, x, c, "fp32")
    _compare(got, _ref(p, h, x, c), "fp32", "fallback")
