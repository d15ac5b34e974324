"""CPU: the training-loop harness (tests/train_loop.py) is the reference's function, the conditions of the GPU test
(tests/test_gpu_train_loop.py) can be met by reference arithmetic alone, and the comparison rejects wrong loops."""
from __future__ import annotations

import functools

import numpy as np
import torch

import prng
import raftdvc_loop as rl
import train_loop as tl
import update_cases as uc
from conftest import grad_inputs, load_golden
from oracle import oracle as orc
from oracle import torch_cpu

FP32_BOUND = lambda iters: (iters + 1) * 1e-5   # noqa: E731  (tests/test_gpu_train_loop.py, "Bounds")
FP32_CAP, CAP_16 = 0.999, 0.99


# ---------------------------------------------------------------------------------------------------------------
# pinned to the reference
# ---------------------------------------------------------------------------------------------------------------
def test_lookup_equals_the_oracle_bit_for_bit():
    """float32, (8, 10, 12) with three levels (no size-1 level): the dtype-preserving restatement and
    oracle/torch_cpu.py (bit-identical to the reference on every golden case) give the same bits."""
    B, C, vol, L, r = 2, 32, (8, 10, 12), 3, 4
    f1, f2 = (torch.from_numpy(prng.normal(s, (B, C) + vol)) for s in (9301, 9302))
    coords = torch.from_numpy(prng.flow_coords(9303, B, *vol, 3.0))
    got = tl.lookup(tl.pyramid(f1, f2, L), coords, r)
    assert got.dtype == torch.float32 and torch.equal(got, torch_cpu.corr_lookup(f1, f2, coords, L, r))
    assert tl.lookup(tl.pyramid(f1.double(), f2.double(), L), coords, r).dtype == torch.float64


def test_lookup_reproduces_the_size_1_level_fixture():
    """grad_edge_888_L4_r4 (8^3, L = 4: level 3 is one voxel): the reference's stored gradients of both feature maps
    within the fixture's standing bound (tests/test_oracle_golden.py: 1e-6), the outputs against the oracle's; the
    size-1 level is all zeros.  In float64 the same level contributes nothing either."""
    g = load_golden("grad_edge_888_L4_r4.npz")
    f1, f2, coords, G, L, r, legacy = grad_inputs(g)
    assert not legacy and L == 4 and f1.shape[2:] == (8, 8, 8)
    n3 = (2 * r + 1) ** 3
    for dt in (torch.float32, torch.float64):
        t1, t2 = (torch.from_numpy(a).to(dt).requires_grad_(True) for a in (f1, f2))
        out = tl.lookup(tl.pyramid(t1, t2, L), torch.from_numpy(coords), r)
        assert out.dtype == dt and not out[:, 3 * n3:].any() and out[:, 2 * n3:3 * n3].any()
        assert orc.rel_err(out.detach().numpy(), orc.corr_lookup(f1, f2, coords, L, r, False)) < 1e-6
        (out * torch.from_numpy(G).to(dt)).sum().backward()
        assert orc.rel_err(t1.grad.numpy(), g["grad_f1"]) < 1e-6 and orc.rel_err(t2.grad.numpy(), g["grad_f2"]) < 1e-6


def test_one_iteration_is_the_update_block():
    """One iteration from the identity grid: the harness's block is raftdvc_loop.update_block on the oracle's lookup,
    bit for bit, its tail is raftdvc_loop.reference_tail, and the loss is the mean end-point error of that flow."""
    leaves, consts, T, _ = tl.case_inputs("A")
    p = {k: t for k, t in leaves.items() if k not in tl.INPUTS}
    coords0 = tl.grid(consts["coords_init"])
    ops, tape = tl.LibraryOps(), tl.Tape()
    cor = ops.cor(tape, ops.corr(leaves["fmap1"], leaves["fmap2"]), coords0, p)
    net, delta, log_b = ops.block(tape, p, leaves["net0"], leaves["context"], coords0 - coords0, cor)
    corr = torch_cpu.corr_lookup(leaves["fmap1"], leaves["fmap2"], coords0, 4, 4)
    wnet, wdelta = rl.update_block(p, leaves["net0"], leaves["context"], coords0 - coords0, corr=corr)
    assert log_b is None and torch.equal(net, wnet) and torch.equal(delta, wdelta)
    assert set(tape.record["masks"]) == {(0, n) for n in tl.RELUS[:-1]}
    _, up, _ = ops.tail(coords0, delta, None, coords0, T)
    _, wup = rl.reference_tail(coords0, wdelta, coords0, T)
    assert torch.equal(up, wup)
    loss, _ = tl.train_loop(ops, leaves["fmap1"], leaves["fmap2"], p, leaves["net0"], leaves["context"], coords0,
                            consts["gt"], T, 1)
    want = (wup.double() - consts["gt"].double()).pow(2).sum(dim=1).sqrt().mean()
    assert abs(float(loss) - float(want)) <= 1e-6 * float(want)


# ---------------------------------------------------------------------------------------------------------------
# the GPU test's conditions can be met
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _float32_against_float64(case="A"):
    leaves, consts, T, iters = tl.case_inputs(case)
    return tl.against_float64(tl.LibraryOps(), leaves, consts, T, iters, "cpu", torch.float32)


def test_float32_meets_the_cap_and_the_bound():
    """The float32 CPU loop as the implementation, the float64 loop on its record, case A: every ReLU's mask agrees on
    >= 0.999 of its elements, the loss and every gradient within (iters + 1) x 1e-5."""
    errs, agree, _, _ = _float32_against_float64()
    iters = tl.CASES["A"][3]
    assert set(agree) == {(i, n) for i in range(iters) for n in tl.RELUS[:-1]}
    print("mask agreement, worst:", min(agree.items(), key=lambda kv: kv[1]))
    print("float32 against float64, worst:", max(errs.items(), key=lambda kv: kv[1]))
    assert min(agree.values()) >= FP32_CAP, agree
    assert len(errs) == 4 + len(uc.params("upd_888")) + 1
    assert max(errs.values()) <= FP32_BOUND(iters), errs


def test_case_b_float32_meets_the_cap_and_the_bound():
    """Case B (two samples, the uncertainty head) in the same way."""
    errs, agree, _, _ = _float32_against_float64("B")
    iters = tl.CASES["B"][3]
    assert set(agree) == {(i, n) for i in range(iters) for n in tl.RELUS}
    print("float32 against float64, worst:", max(errs.items(), key=lambda kv: kv[1]))
    assert min(agree.values()) >= FP32_CAP, agree
    assert max(errs.values()) <= FP32_BOUND(iters), errs


def test_bfloat16_autocast_meets_the_cap():
    """The update block and convc1 under torch.autocast("cpu", torch.bfloat16) as the implementation: >= 0.99."""
    leaves, consts, T, iters = tl.case_inputs("A")
    ops = tl.LibraryOps(autocast=("cpu", torch.bfloat16))
    errs, agree, _, _ = tl.against_float64(ops, leaves, consts, T, iters, "cpu", torch.float32)
    print("mask agreement, worst:", min(agree.items(), key=lambda kv: kv[1]))
    print("bfloat16 autocast against float64, worst:", max(errs.items(), key=lambda kv: kv[1]))
    assert min(agree.values()) >= CAP_16, agree
    assert all(np.isfinite(v) for v in errs.values())


# ---------------------------------------------------------------------------------------------------------------
# the test has power
# ---------------------------------------------------------------------------------------------------------------
class _NetDetached(tl.LibraryOps):
    """The hidden state carries no gradient from iteration i + 1 back into iteration i."""

    def block(self, tape, p, net, context, flow, cor):
        return super().block(tape, p, net.detach() if tape.it else net, context, flow, cor)


class _StaleSavedTensors(tl.LibraryOps):
    """Iteration 1 runs on what iteration 0 kept: its convc1 mask and its GRU input (an overwritten saved tensor)."""

    def cor(self, tape, corr, coords1, p):
        if tape.it != 1:
            return super().cor(tape, corr, coords1, p)
        pre = rl._conv(p, "encoder.convc1", tl.lookup(corr, coords1, self.radius), 0)
        return tape.seen("convc1", pre * tape.record["masks"][(0, "convc1")].to(pre.dtype))

    def gru_input(self, tape, p, context, flow, cor):
        inp = super().gru_input(tape, p, context, flow, cor)
        if tape.it == 0:
            self._kept = inp
        return self._kept if tape.it == 1 else inp


def _rejected(ops, name, gamma=0.8):
    leaves, consts, T, iters = tl.case_inputs("A")
    errs, _, _, _ = tl.against_float64(ops, leaves, consts, T, iters, "cpu", torch.float32, gamma=gamma)
    print(type(ops).__name__, "gamma", gamma, name, f"{errs[name]:.2e}", "worst",
          max(errs.items(), key=lambda kv: kv[1]))
    assert errs[name] >= 100 * FP32_BOUND(iters), (name, errs[name])


def test_a_detached_hidden_state_is_rejected():
    _rejected(_NetDetached(), "net0")


def test_stale_saved_tensors_are_rejected():
    _rejected(_StaleSavedTensors(), "encoder.convc1.weight")


def test_an_ignored_gamma_is_rejected():
    _rejected(tl.LibraryOps(), "flow_head.conv2.bias", gamma=1.0)


def test_an_optimiser_step_moves_every_gradient():
    """The float64 loop before and after sgd_step (parameters and both feature maps): every parameter's gradient moves
    by >= 100 x the fp32 bound, so a pack left over from before the step cannot pass test_two_optimiser_steps."""
    leaves, consts, T, iters = tl.case_inputs("A")
    lv = {k: t.double() for k, t in leaves.items()}
    _, before, _ = tl.run(tl.LibraryOps(), lv, consts, T, iters, "cpu", torch.float64)
    moved = {k: t.clone() for k, t in lv.items()}
    tl.sgd_step({k: t for k, t in moved.items() if k not in ("net0", "context")}, before)
    for k in moved:
        if k not in ("net0", "context"):
            step = (moved[k] - lv[k]).abs().max() / lv[k].abs().max()
            assert abs(float(step) - 0.1) < 1e-12, (k, float(step))
    _, after, _ = tl.run(tl.LibraryOps(), moved, consts, T, iters, "cpu", torch.float64)
    change = {k: uc.err(after[k], before[k]) for k in before if k not in tl.INPUTS}
    print("least moved:", min(change.items(), key=lambda kv: kv[1]))
    assert min(change.values()) >= 100 * FP32_BOUND(iters), change
