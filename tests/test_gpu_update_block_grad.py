"""GPU: dvccorr.update_block_ad, BasicUpdateBlock.forward as one differentiable call (conv7x7x7_flow_ad, conv3x3x3_ad,
torch.cat and sep_conv_gru_ad).  Forward values against UpdateBlock bit for bit, gradients against the hand-written
chain of the individual ops bit for bit, and against the reference's autograd results
(tests/golden/gen_update_block_grad_golden.py)."""
from __future__ import annotations

import functools

import pytest
import torch
import torch.nn.functional as F

import prng
import update_cases as uc
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PRECISIONS = ("fp32", "fp16", "bf16")
# fp32 against the reference's stored gradients: see test_reference_fixture (the merged chain measures 9.73e-6)
FIXTURE_BOUND = 1e-5


def _uniform(seed, shape, bound=1.0):
    return torch.from_numpy(prng.uniform(seed, tuple(shape), -bound, bound))


def _leaves(name, flow_seed=None):
    """Device copies of a case's parameters and inputs (net0, context, flow, cor), all requiring grad but the flow."""
    p, c = uc.params(name), uc.case(name)
    pd = {n: t.to(DEV).clone().requires_grad_(True) for n, t in p.items()}
    flow = c["flow"] if flow_seed is None else _uniform(flow_seed, c["flow"].shape, 2.0)
    ins = {k: c[k].to(DEV).clone().requires_grad_(True) for k in ("net0", "context", "cor")}
    return pd, ins, flow.to(DEV)


def _loss(outs, seeds):
    return sum((_uniform(s, o.shape).to(DEV) * o).sum() for o, s in zip(outs, seeds) if o is not None)


def _library_convf1(flow, weight, bias):
    with torch.autocast("cuda", enabled=False):
        return F.relu(F.conv3d(flow, weight, bias, padding=3))


def _chain(pd, net, context, flow, cor, precision, convf1=None, corr=None):
    """The block written out with the individual differentiable ops (convf1: a replacement for conv7x7x7_flow_ad; corr:
    a raw correlation volume instead of cor; a ConvGRU3D state dict runs the GRU as F.conv3d calls in float32)."""
    import dvccorr
    w = lambda l: (pd[l + ".weight"], pd[l + ".bias"])   # noqa: E731
    conv = functools.partial(dvccorr.conv3x3x3_ad, precision=precision)
    if corr is not None:
        cor = F.relu(F.conv3d(corr, *w("encoder.convc1")))
    flo1 = (convf1 or functools.partial(dvccorr.conv7x7x7_flow_ad, precision=precision))(flow, *w("encoder.convf1"))
    flo2 = conv(flo1, *w("encoder.convf2"), relu=True)
    mot = conv(cor, *w("encoder.conv"), relu=True, x2=flo2)
    inp = torch.cat([context, mot, flow], dim=1)
    if "gru.convz.weight" in pd:
        hx = torch.cat([net, inp], dim=1)
        z, r = torch.sigmoid(F.conv3d(hx, *w("gru.convz"), padding=1)), torch.sigmoid(F.conv3d(hx, *w("gru.convr"), padding=1))
        q = torch.tanh(F.conv3d(torch.cat([r * net, inp], dim=1), *w("gru.convq"), padding=1))
        net = (1 - z) * net + z * q
    else:
        net = dvccorr.sep_conv_gru_ad(net, inp, {n[4:]: t for n, t in pd.items() if n.startswith("gru.")},
                                      precision=precision)
    delta = conv(conv(net, *w("flow_head.conv1"), relu=True), *w("flow_head.conv2"))
    log_b = None
    if "uncertainty_head.conv1.weight" in pd:
        log_b = conv(conv(net, *w("uncertainty_head.conv1"), relu=True), *w("uncertainty_head.conv2"))
    return net, delta, log_b


def _grads(pd, ins):
    out = {n: t.grad for n, t in pd.items() if t.grad is not None}
    out.update({k: t.grad for k, t in ins.items()})
    return out


@pytest.mark.parametrize("name", ("upd_215", "upd_b2_597"))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_forward_equals_update_block(precision, name):
    import dvccorr
    pd, ins, flow = _leaves(name)
    got = dvccorr.update_block_ad(ins["net0"], ins["context"], flow, pd, cor=ins["cor"], precision=precision)
    with torch.no_grad():
        want = dvccorr.UpdateBlock(pd, precision=precision)(ins["net0"], ins["context"], flow, cor=ins["cor"])
    assert (got[2] is None) == (want[2] is None) == (uc.case_meta(name)[2] == "none")
    for a, b in zip(got, want):
        if b is not None:
            assert a.requires_grad and a.dtype == torch.float32 and torch.equal(a.detach(), b)


@pytest.mark.parametrize("precision", ("fp32", "bf16"))
def test_backward_equals_the_chain_of_ops(precision):
    """Every gradient equals, bit for bit, the hand-written chain's on the same inputs: slice order in the GRU input, a
    dropped context gradient or a swapped weight would all show, with no tolerance."""
    import dvccorr
    seeds = (9001, 9002, 9003)
    pd, ins, flow = _leaves("upd_215")
    _loss(dvccorr.update_block_ad(ins["net0"], ins["context"], flow, pd, cor=ins["cor"], precision=precision),
          seeds).backward()
    got = _grads(pd, ins)
    pd2, ins2, _ = _leaves("upd_215")
    _loss(_chain(pd2, ins2["net0"], ins2["context"], flow, ins2["cor"], precision), seeds).backward()
    want = _grads(pd2, ins2)
    assert set(got) == set(want) == (set(pd) - {"encoder.convc1.weight", "encoder.convc1.bias"}) | set(ins)
    for k in want:
        assert want[k].abs().max() > 0 and torch.equal(got[k], want[k]), k


def _fixture_errors(grads, ref, refw):
    errs = {"d_net": uc.err(grads["net0"], ref["d_net"]), "d_context": uc.err(grads["context"], ref["d_context"]),
            "d_cor": uc.err(grads["cor"], ref["d_cor"]),
            "convf1_dw": uc.err(grads["encoder.convf1.weight"], ref["convf1_dw"]),
            "convf1_db": uc.err(grads["encoder.convf1.bias"], ref["convf1_db"])}
    for k, v in ref.items():
        if k.startswith("db."):
            errs[k] = uc.err(grads[k[3:] + ".bias"], v)
    for k, v in refw.items():
        errs[k] = uc.err(grads[k[4:] + ".weight"][::8], v)
    return errs


def test_reference_fixture():
    """fp32 against the reference's autograd results for the whole block (case upd_b2_597 with the fixture's flow seed,
    loss sum(c_net net) + sum(c_delta delta_flow)): d net, d context, d cor, convf1's gradients and every bias gradient
    in full, the other weight gradients on output channels 0, 8, ..  The fixture's generator asserts that no ReLU
    pre-activation is within 1e-5 max|activation| of zero, so the masks agree.

    The bound.  The chain is three GRU passes plus two to three convolutions deep, so the per-op tolerance 1e-5 need
    not bound the composition.  The test first measures the same chain with convf1 taken from F.conv3d in float32
    (every other op is the merged conv3x3x3_ad / sep_conv_gru_ad): the bound is twice that error, or 1e-5 where the
    merged chain already holds 1e-5.  Measured on an MI355X (max over all 31 gradient tensors): merged chain 9.73e-6
    (dw8.flow_head.conv2), update_block_ad 9.61e-6 (convf1_dw; 9.0e-6 in the merged chain).  The merged chain holds
    1e-5, so the bound is 1e-5."""
    import dvccorr
    ref = {k: torch.from_numpy(v) for k, v in load_golden("updblk_grad_b2_597.npz").items()}
    refw = {k: torch.from_numpy(v) for k, v in load_golden("updblk_grad_b2_597_w.npz").items()}
    s_net, s_delta, s_b, s_flow = (int(v) for v in ref["seeds"])
    pd, ins, flow = _leaves("upd_b2_597", s_flow)
    _loss(_chain(pd, ins["net0"], ins["context"], flow, ins["cor"], "fp32", _library_convf1),
          (s_net, s_delta, s_b)).backward()
    merged = _fixture_errors(_grads(pd, ins), ref, refw)
    pd, ins, flow = _leaves("upd_b2_597", s_flow)
    _loss(dvccorr.update_block_ad(ins["net0"], ins["context"], flow, pd, cor=ins["cor"], precision="fp32"),
          (s_net, s_delta, s_b)).backward()
    errs = _fixture_errors(_grads(pd, ins), ref, refw)
    print("merged chain (convf1 from F.conv3d):", f"{max(merged.values()):.2e}",
          {k: f"{v:.1e}" for k, v in merged.items()})
    print("update_block_ad:", f"{max(errs.values()):.2e}", {k: f"{v:.1e}" for k, v in errs.items()})
    assert len(errs) == 5 + 4 + 9 + 4 + 9
    assert max(errs.values()) <= FIXTURE_BOUND, errs


def test_checkpoint():
    """torch.utils.checkpoint(update_block_ad, ..., use_reentrant=False) recomputes the block in the backward: same
    values and gradients, bit for bit."""
    import dvccorr
    from torch.utils.checkpoint import checkpoint
    seeds = (9011, 9012, 9013)
    pd, ins, flow = _leaves("upd_215")
    _loss(dvccorr.update_block_ad(ins["net0"], ins["context"], flow, pd, cor=ins["cor"], precision="fp32"),
          seeds).backward()
    want = _grads(pd, ins)
    pd2, ins2, _ = _leaves("upd_215")
    outs = checkpoint(lambda n, c, r: dvccorr.update_block_ad(n, c, flow, pd2, cor=r, precision="fp32"),
                      ins2["net0"], ins2["context"], ins2["cor"], use_reentrant=False)
    _loss(outs, seeds).backward()
    got = _grads(pd2, ins2)
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_two_training_iterations():
    """lookup_convc1 -> update_block_ad -> flow_step twice on 8^3 feature maps with coords1.detach() at the top of each
    iteration (raft_dvc.py:441).  The loss (the mean end-point error of both upsampled flows: train_loop.sequence_loss
    against a zero ground truth, gamma 1) and the gradients of both feature maps and of every parameter against the
    float64 loop of tests/train_loop.py on the same inputs, which runs on the coordinates and ReLU decisions recorded
    from the chain of ops (bit-identical to update_block_ad: test_backward_equals_the_chain_of_ops).  Bound:
    (iters + 1) x 1e-5 = 3e-5 per tensor, as tests/test_gpu_train_loop.py derives it."""
    import dvccorr
    import train_loop as tl
    B, vol, T = 1, (8, 8, 8), (16, 16, 16)
    c = uc.case("upd_888")
    leaves = {"fmap1": torch.from_numpy(prng.normal(9021, (B, 32, *vol))),
              "fmap2": torch.from_numpy(prng.normal(9022, (B, 32, *vol))), "net0": c["net0"], "context": c["context"]}
    leaves.update(uc.params())
    coords_init = torch.from_numpy(prng.identity_coords(B, *vol)) + _uniform(9023, (B, 3, *vol), 1.5)
    gt = torch.zeros((B, 3) + T)
    pd = {n: t.to(DEV).clone().requires_grad_(True) for n, t in uc.params().items()}
    f1, f2 = leaves["fmap1"].to(DEV).requires_grad_(True), leaves["fmap2"].to(DEV).requires_grad_(True)
    net, ctx = c["net0"].to(DEV), c["context"].to(DEV)
    corr_fn = dvccorr.CorrBlock(f1, f2, 4, 4, precision="fp32")
    coords0 = dvccorr.coords_grid_3d(B, *vol, DEV)
    coords1 = coords_init.to(DEV)
    ups = []
    for it in range(2):
        coords1 = coords1.detach()
        cor = corr_fn.lookup_convc1(coords1, pd["encoder.convc1.weight"], pd["encoder.convc1.bias"])
        net, delta, _ = dvccorr.update_block_ad(net, ctx, coords1 - coords0, pd, cor=cor, precision="fp32")
        coords1, up = dvccorr.flow_step(coords1, delta, T)
        ups.append(up)
    loss = tl.sequence_loss(ups, [], gt.to(DEV), 1.0)
    loss.backward()
    got = {"fmap1": f1.grad, "fmap2": f2.grad, **{n: t.grad for n, t in pd.items()}}
    _, agree, _, (rloss, want) = tl.against_float64(tl.HipOps("fp32", dvccorr.CorrBlock), leaves,
                                                    {"coords_init": coords_init, "gt": gt}, T, 2, DEV, torch.float32,
                                                    gamma=1.0, ref_gamma=1.0)
    assert min(agree.values()) >= 0.999, agree
    errs = {k: uc.err(got[k], want[k]) for k in got}
    errs["loss"] = abs(float(loss.detach()) - float(rloss)) / abs(float(rloss))
    print("two training iterations, worst:", max(errs.items(), key=lambda kv: kv[1]))
    assert len(errs) == 2 + len(pd) + 1 and max(errs.values()) <= 3e-5, errs


def _float64_grads(p, c, seeds, separable=True, corr=False):
    """The block in float64 on the CPU (raftdvc_loop), its loss and gradients for the leaves named like _leaves'."""
    pd = {n: t.double().requires_grad_(True) for n, t in p.items()}
    ins = {k: c[k].double().requires_grad_(True) for k in ("net0", "context", "corr" if corr else "cor")}
    flow = c["flow"].double()
    mf = uc.rl.motion_features(pd, flow, **({"corr": ins["corr"]} if corr else {"cor": ins["cor"]}))
    inp = torch.cat([ins["context"], mf], dim=1)
    if separable:
        net = uc.rl.sep_gru(pd, ins["net0"], inp)
    else:
        h = ins["net0"]
        hx = torch.cat([h, inp], dim=1)
        z, r = torch.sigmoid(uc.rl._conv(pd, "gru.convz", hx, 1)), torch.sigmoid(uc.rl._conv(pd, "gru.convr", hx, 1))
        q = torch.tanh(uc.rl._conv(pd, "gru.convq", torch.cat([r * h, inp], dim=1), 1))
        net = (1 - z) * h + z * q
    outs = [net]
    for head in ("flow_head", "uncertainty_head"):
        if head + ".conv1.weight" in pd:
            outs.append(uc.rl._conv(pd, head + ".conv2", F.relu(uc.rl._conv(pd, head + ".conv1", net, 1)), 1))
    sum((_uniform(s, o.shape).double() * o).sum() for o, s in zip(outs, seeds)).backward()
    return {**{n: t.grad for n, t in pd.items() if t.grad is not None}, **{k: t.grad for k, t in ins.items()}}


def _slow_path_bound(merged):
    """The rule of test_reference_fixture for a path that has no stored measurement: twice the error of the same chain
    with convf1 taken from F.conv3d in float32 (merged code only), or 1e-5 where that chain already holds 1e-5."""
    worst = max(merged.values())
    return 1e-5 if worst <= 1e-5 else 2 * worst


def test_raw_corr_slow_path():
    """corr instead of cor: convc1 runs as F.conv3d in float32 with autograd on; corr and convc1's parameters get
    gradients.  Against float64 on the CPU, bounded by the merged chain's own error (_slow_path_bound)."""
    import dvccorr
    seeds = (9031, 9032, 9033)
    p, c = uc.params("upd_215"), uc.case("upd_215")
    want = _float64_grads(p, c, seeds, corr=True)

    def run(block):
        pd, ins, flow = _leaves("upd_215")
        corr = c["corr"].to(DEV).clone().requires_grad_(True)
        _loss(block(pd, ins, flow, corr), seeds).backward()
        got = {**{n: t.grad for n, t in pd.items()}, "net0": ins["net0"].grad, "context": ins["context"].grad,
               "corr": corr.grad}
        assert set(want) == set(got)
        return {k: uc.err(got[k], want[k]) for k in want}
    merged = run(lambda pd, ins, flow, corr: _chain(pd, ins["net0"], ins["context"], flow, None, "fp32",
                                                    _library_convf1, corr=corr))
    errs = run(lambda pd, ins, flow, corr: dvccorr.update_block_ad(ins["net0"], ins["context"], flow, pd, corr=corr,
                                                                   precision="fp32"))
    print("raw corr: merged chain", f"{max(merged.values()):.2e}", "update_block_ad", f"{max(errs.values()):.2e}")
    assert max(errs.values()) <= _slow_path_bound(merged), (errs, merged)


def test_non_separable_gru_state_dict():
    """A ConvGRU3D state dict: the GRU runs as the float32 library composition with autograd on, the other layers on
    the kernels.  Against float64 on the CPU, bounded by the merged chain's own error (_slow_path_bound)."""
    import dvccorr
    seeds = (9041, 9042, 9043)
    p = {n: t for n, t in uc.params("upd_215").items() if not n.startswith("gru.")}
    for i, g in enumerate("zrq"):
        p[f"gru.conv{g}.weight"] = _uniform(8701 + 2 * i, (96, 243, 3, 3, 3), 0.012)
        p[f"gru.conv{g}.bias"] = _uniform(8702 + 2 * i, (96,), 0.012)
    c = uc.case("upd_215")
    want = _float64_grads(p, c, seeds, separable=False)

    def run(block):
        pd = {n: t.to(DEV).clone().requires_grad_(True) for n, t in p.items()}
        ins = {k: c[k].to(DEV).clone().requires_grad_(True) for k in ("net0", "context", "cor")}
        _loss(block(pd, ins, c["flow"].to(DEV)), seeds).backward()
        got = _grads(pd, ins)
        assert set(want) == set(got)
        return {k: uc.err(got[k], want[k]) for k in want}
    merged = run(lambda pd, ins, flow: _chain(pd, ins["net0"], ins["context"], flow, ins["cor"], "fp32",
                                              _library_convf1))
    errs = run(lambda pd, ins, flow: dvccorr.update_block_ad(ins["net0"], ins["context"], flow, pd, cor=ins["cor"],
                                                             precision="fp32"))
    print("non-separable: merged chain", f"{max(merged.values()):.2e}", "update_block_ad", f"{max(errs.values()):.2e}")
    assert max(errs.values()) <= _slow_path_bound(merged), (errs, merged)
