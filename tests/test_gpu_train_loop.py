"""GPU: the refinement loop of RAFTDVC.forward (raft_dvc.py:440-491) under autograd with the sequence loss on top and
two optimiser steps, on dvccorr's differentiable ops (lookup_convc1, conv7x7x7_flow_ad, conv3x3x3_ad, sep_conv_gru_ad,
update_block_ad, flow_step, upflow_3d), gradient by gradient against a float64 restatement on the CPU
(tests/train_loop.py, pinned to the reference by tests/test_train_loop_cpu.py).

What a single-call gradient test cannot see and this one does: state saved by iteration i and overwritten by iteration
i + 1 before the backward runs; contributions of the T iterations to d fmap1 / d fmap2 / d convc1 and to every
update-block parameter that are dropped, doubled or computed from another iteration's saved tensors; the gradient that
`net` carries from iteration i + 1 back into iteration i; a weight pack left over from before an in-place optimiser
step (forward, dgrad, GRU, convc1, convf1 packs); the size-1 pyramid level inside a training loop; batch indexing
across the composition.

How the comparison is made well-posed: see tests/train_loop.py (the implementation records its detached coords1_i and
the decision act > 0 of every ReLU; the float64 loop runs on that record and reports how often its own pre > 0 agrees).
The caps on that agreement are conditions of the test, not a way to skip elements: fp32 >= 0.999, 16-bit >= 0.99 per
ReLU and iteration.

Cases: A  B = 1, 32 x (8, 10, 12) feature maps (levels 8.10.12, 4.5.6, 2.2.3, 1.1.1: a zero level, partial tiles on all
three axes), target (61, 77, 93), 3 iterations, no uncertainty head;  B  B = 2, 32 x 8^3, target 64^3, 2 iterations,
the uncertainty head (update_meta.json's parameters), so _UpflowFn's backward runs inside the loop.
Leaves compared: fmap1, fmap2, net0, context and every parameter, convc1's included; metric update_cases.err.

Bounds.
  fp32: one update_block_ad call holds 1e-5 against the reference's autograd (FIXTURE_BOUND), lookup_convc1_ad holds
    1e-5 (TOL["fp32"]); to first order the errors of `iters` chained blocks and of the lookup add: (iters + 1) x 1e-5
    per tensor and for the loss.
  fp16 / bf16: the yardstick is the reference's own AMP arithmetic: the same loop on the GPU with convc1 and the update
    block as library calls under torch.autocast of that dtype, the correlation as the restated lookup in float32 (the
    reference builds it outside autocast; oracle/torch_cpu.py itself divides by S - 1 = 0 at the size-1 level).  The
    yardstick records its own coordinates and masks and is compared with float64 on its own record; the HIP error per
    tensor may be at most 2 x the yardstick's on that tensor (equal operand precision, another summation order: the
    form and margin of test_gpu_encoder.py and the EPE tests).  The loss is one scalar, whose yardstick error can be
    small by coincidence: its bound is 2 x max(yardstick's loss error, the format's unit roundoff 2^-8 / 2^-11).
    fp16 runs both sides with the loss scaled by 1024 (the reference trains with a GradScaler; conv3x3x3_ad rounds the
    incoming gradient to fp16).

Measured on an MI355X: DESIGN.md 4.16.
"""
from __future__ import annotations

import functools

import pytest
import torch

import train_loop as tl

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
COMBOS = {"fp32": "CorrBlock", "fp16": "CorrBlock", "bf16": "CorrBlockFused"}
AMP_DTYPE = {"fp16": torch.float16, "bf16": torch.bfloat16}
ROUNDOFF = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8}
LOSS_SCALE = {"fp32": 1.0, "fp16": 1024.0, "bf16": 1.0}
CAP = {"fp32": 0.999, "fp16": 0.99, "bf16": 0.99}


def fp32_bound(iters):
    return (iters + 1) * 1e-5


def _hip(precision, **kw):
    import dvccorr
    return tl.HipOps(precision, getattr(dvccorr, COMBOS[precision]), **kw)


def _yardstick(precision):
    return tl.LibraryOps(autocast=("cuda", AMP_DTYPE[precision]))


@functools.lru_cache(maxsize=None)
def _chain_run(case, precision):
    """The HIP chain loop (recording) and the float64 reference on its record: shared, callers must not modify it."""
    leaves, consts, T, iters = tl.case_inputs(case)
    return tl.against_float64(_hip(precision), leaves, consts, T, iters, DEV, torch.float32,
                              loss_scale=LOSS_SCALE[precision])


@functools.lru_cache(maxsize=None)
def _block_ad_run(precision):
    leaves, consts, T, iters = tl.case_inputs("A")
    loss, grads, _ = tl.run(_hip(precision, fused_block=True), leaves, consts, T, iters, DEV, torch.float32,
                            loss_scale=LOSS_SCALE[precision])
    return loss, grads


def _report(what, errs, agree):
    worst = max(errs.items(), key=lambda kv: kv[1])
    low = min(agree.items(), key=lambda kv: kv[1])
    print(f"{what}: worst {worst[0]} {worst[1]:.2e}; loss {errs['loss']:.2e}; mask agreement >= {low[1]:.5f} {low[0]}")


def _check(precision, iters, errs, agree, yard):
    """The caps, then the bound per tensor and for the loss (module docstring); yard = the yardstick's (errs, agree)."""
    assert min(agree.values()) >= CAP[precision], agree
    if precision == "fp32":
        bound = {k: fp32_bound(iters) for k in errs}
    else:
        yerrs, yagree = yard
        assert min(yagree.values()) >= CAP[precision], yagree
        bound = {k: 2 * v for k, v in yerrs.items()}
        bound["loss"] = 2 * max(yerrs["loss"], ROUNDOFF[precision])
        print({k: (f"{errs[k]:.2e}", f"{yerrs[k]:.2e}") for k in errs})
    over = {k: (errs[k], bound[k]) for k in errs if not errs[k] <= bound[k]}
    assert not over, over


@pytest.mark.parametrize("precision", tuple(COMBOS))
@pytest.mark.parametrize("case", tuple(tl.CASES))
def test_loop_gradients(case, precision):
    """The loss and every gradient of the T-iteration loop on the HIP ops against float64.

    Measured on an MI355X, worst tensor, HIP (yardstick on that tensor), and the largest HIP / yardstick ratio:
      A fp32 fmap2 8.63e-6 (bound 4e-5)                  B fp32 fmap1 9.71e-6 (bound 3e-5)
      A fp16 encoder.convc1.weight 6.55e-4 (6.27e-4), 1.04    B fp16 encoder.convf1.weight 7.03e-4 (9.89e-4), 1.19
      A bf16 encoder.convf1.weight 5.80e-3 (5.56e-3), 1.32    B bf16 encoder.convc1.weight 5.33e-3 (6.54e-3), 1.11
    Mask agreement >= 0.99997 (fp32), 0.99980 (fp16), 0.99872 (bf16).  The whole table: DESIGN.md 4.16."""
    leaves, consts, T, iters = tl.case_inputs(case)
    errs, agree, _, _ = _chain_run(case, precision)
    has_unc = any(k.startswith("uncertainty_head.") for k in leaves)
    assert set(agree) == {(i, n) for i in range(iters) for n in tl.RELUS[:6 if has_unc else 5]}
    assert set(errs) == set(leaves) | {"loss"}
    _report(f"{case} {precision} HIP", errs, agree)
    yard = None
    if precision != "fp32":
        yard = tl.against_float64(_yardstick(precision), leaves, consts, T, iters, DEV, torch.float32,
                                  loss_scale=LOSS_SCALE[precision])[:2]
        _report(f"{case} {precision} autocast yardstick", *yard)
    _check(precision, iters, errs, agree, yard)


@pytest.mark.parametrize("precision", ("fp32", "bf16"))
def test_update_block_ad_equals_chain_in_the_loop(precision):
    """The same loop with update_block_ad in place of the chain of ops, case A: the loss and every gradient bit for
    bit, over three iterations that share the pack cache and the GRU's saved tensors."""
    _, _, (closs, cgrads), _ = _chain_run("A", precision)
    loss, grads = _block_ad_run(precision)
    assert torch.equal(loss, closs)
    assert set(grads) == set(cgrads)
    for k in cgrads:
        assert torch.equal(grads[k], cgrads[k]), k


def _two_steps(ops, precision):
    """Two training steps of case A with sgd_step between them on both sides (each side takes its own step-1
    gradients, in place, on every parameter and both feature maps; the same tensor objects go into step 2, the
    correlation block is rebuilt from the updated maps).  Returns step 2's (errors, agreement)."""
    leaves, consts, T, iters = tl.case_inputs("A")
    dev = {k: t.to(DEV).clone().requires_grad_(True) for k, t in leaves.items()}
    ref = {k: t.double().clone().requires_grad_(True) for k, t in leaves.items()}
    stepped = lambda d: {k: t for k, t in d.items() if k not in ("net0", "context")}   # noqa: E731
    for step in range(2):
        loss, grads, record = tl.run(ops, dev, consts, T, iters, DEV, torch.float32, loss_scale=LOSS_SCALE[precision])
        rloss, rgrads, record = tl.run(tl.LibraryOps(), ref, consts, T, iters, "cpu", torch.float64, record=record)
        if step == 0:
            tl.sgd_step(stepped(dev), grads)
            tl.sgd_step(stepped(ref), rgrads)
    return tl.errors((loss, grads), (rloss, rgrads)), record["agreement"]


@pytest.mark.parametrize("precision", ("fp32", "bf16"))
def test_two_optimiser_steps(precision):
    """Step 2 after an in-place optimiser step that moves every tensor by a tenth of its largest entry: a pack left
    over from step 1 (forward, dgrad, GRU, convc1, convf1) is a 10 % error in the gradients
    (test_train_loop_cpu.py::test_an_optimiser_step_moves_every_gradient).  Step-2 gradients within the bound of the
    float64 side's step 2, which runs on step 2's own record; and the conv3 pack cache holds no more entries than
    there are (layer, kind) pairs, i.e. it does not grow per call or per step."""
    from dvccorr import library
    library._conv3_packs()._entries.clear()
    errs, agree = _two_steps(_hip(precision), precision)
    entries = len(library._conv3_packs()._entries)
    _report(f"step 2 {precision} HIP", errs, agree)
    yard = None
    if precision != "fp32":
        yard = _two_steps(_yardstick(precision), precision)
        _report(f"step 2 {precision} autocast yardstick", *yard)
    _check(precision, tl.CASES["A"][3], errs, agree, yard)
    # forward and dgrad packs of convf2, encoder.conv, flow_head.conv1 / conv2; convf1's; the GRU's forward and dgrad
    assert 0 < entries <= 2 * 4 + 1 + 2, entries


def test_upflow_adjoint_is_reproducible():
    """What the bit-for-bit tests of the loop stand on: the adjoint of upflow_3d sums in a fixed order (no atomic
    scatter), on case A's ceil-shaped target and on one with a size-1 source axis."""
    from dvccorr import corr_block
    for lo, hi in (((1, 3, 8, 10, 12), (61, 77, 93)), ((2, 4, 3, 1, 5), (9, 4, 15))):
        g = torch.randn(lo[:2] + hi, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
        first = corr_block._upflow_adjoint(g, lo)
        assert first.shape == lo and torch.equal(first, corr_block._upflow_adjoint(g, lo))
        want = torch.ops.aten.upsample_trilinear3d_backward(
            g * torch.tensor([hi[i] / lo[2 + i] for i in range(3)] + [1.0] * (lo[1] - 3), device=DEV).view(1, -1, 1, 1, 1),
            list(hi), list(lo), True, None, None, None)
        assert float((first - want).abs().max() / want.abs().max()) <= 1e-5   # two float32 summation orders


def test_checkpointed_loop():
    """torch.utils.checkpoint(..., use_reentrant=False) around lookup_convc1 and around update_block_ad (the
    reference's checkpoint_corr / checkpoint_updates, raft_dvc.py:446-475): each iteration is recomputed in the
    backward, after the later iterations ran their forward.  The loss and every gradient bit for bit."""
    leaves, consts, T, iters = tl.case_inputs("A")
    want_loss, want = _block_ad_run("fp32")
    loss, grads, _ = tl.run(_hip("fp32", fused_block=True, checkpoint=True), leaves, consts, T, iters, DEV,
                            torch.float32)
    assert torch.equal(loss, want_loss)
    for k in want:
        assert torch.equal(grads[k], want[k]), k
