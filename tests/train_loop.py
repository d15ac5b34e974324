"""Test-only harness: RAFT-DVC's refinement loop under autograd with the sequence loss on top, for the closed-loop
gradient check (tests/test_train_loop_cpu.py, tests/test_gpu_train_loop.py).  TEST INFRASTRUCTURE, never product code.

Restates the reference's math (zachtong/RAFT-DVC) beside raftdvc_loop.py:
  CorrBlock                    src/core/corr.py:41-63, 116-208   pyramid and lookup in the dtype of the feature maps
                                                                 (oracle/torch_cpu.py ends in .float() and has no rule
                                                                 for a level with a size-1 axis: such a level samples
                                                                 zeros and carries no gradient)
  refinement loop              src/core/raft_dvc.py:440-491      coords1.detach(); corr_fn(coords1); update block;
                                                                 coords1 += delta; upflow_3d of the flow and of log_b
  SequenceLoss                 src/training/loss.py:66-124       sum_i gamma^(n-i-1) mean_voxels epe(up_i, gt)

One loop body (train_loop) serves every side of the comparison through an `ops` object: the float64 / float32 CPU
reference and the autocast yardstick (LibraryOps) and the HIP ops (HipOps).  What makes a float64 loop comparable with a
float32 or 16-bit one at a per-op tolerance:
  * coords1 is detached at the top of every iteration, so per iteration it is a constant of the differentiated function:
    the implementation under test RECORDS its coords1_i and the reference looks up at the same coordinates.  The
    reference still computes its own net, delta_i and up_i; `net` is the only differentiable state crossing iterations.
  * every ReLU decision is taken from the implementation's own output (act > 0, as tests/test_gpu_proj_grad.py does for
    one op): the reference differentiates pre * mask and reports how often its own pre > 0 agrees with the mask.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

import prng
import raftdvc_loop as rl

RELUS = ("convc1", "convf1", "convf2", "encoder.conv", "flow_head.conv1", "uncertainty_head.conv1")
LOG_B_SEED = 9400      # + iteration: the coefficients of the linear functional of log_b_up


# ---------------------------------------------------------------------------------------------------------------
# the correlation block, dtype preserving (corr.py:116-208)
# ---------------------------------------------------------------------------------------------------------------
def pyramid(fmap1, fmap2, num_levels):
    """corr.py:136-167: (B*N, 1, H_l, W_l, D_l) per level, in the dtype of the feature maps."""
    B, C, H, W, D = fmap1.shape
    N = H * W * D
    cost = torch.matmul(fmap1.reshape(B, C, N).transpose(1, 2), fmap2.reshape(B, C, N))
    cost = cost / torch.sqrt(torch.tensor(C, dtype=cost.dtype, device=cost.device))
    level = cost.reshape(B * N, 1, H, W, D)
    out = [level]
    for _ in range(num_levels - 1):
        level = F.avg_pool3d(level, 2, stride=2)
        out.append(level)
    return out


def _sample(vol, pts):
    """corr.py:41-63 (fixed convention): vol (M, 1, S_h, S_w, S_d); pts (M, n, n, n, 3) in (h, w, d) order.  A volume
    with a size-1 axis divides by S - 1 = 0 there; the reference then samples all zeros: zeros and no gradient here."""
    M, _, Sh, Sw, Sd = vol.shape
    if min(Sh, Sw, Sd) == 1:
        return vol.new_zeros((M, 1) + tuple(pts.shape[1:4]))
    g = pts.clone()
    g[..., 0] = 2.0 * g[..., 0] / (Sh - 1) - 1.0
    g[..., 1] = 2.0 * g[..., 1] / (Sw - 1) - 1.0
    g[..., 2] = 2.0 * g[..., 2] / (Sd - 1) - 1.0
    g = g[..., [1, 0, 2]].permute(0, 3, 1, 2, 4)
    res = F.grid_sample(vol.permute(0, 1, 4, 2, 3), g, mode="bilinear", padding_mode="zeros", align_corners=True)
    return res.permute(0, 1, 3, 4, 2)


def lookup(pyr, coords, radius):
    """corr.py:169-208 without the closing .float(): coords (B, 3, H, W, D) -> (B, L (2r+1)^3, H, W, D)."""
    B, _, H, W, D = coords.shape
    N = H * W * D
    dt, dev = pyr[0].dtype, pyr[0].device
    cr = coords.to(dt).reshape(B, 3, N).permute(0, 2, 1).reshape(B * N, 1, 1, 1, 3)
    n = 2 * radius + 1
    steps = torch.linspace(-radius, radius, n, device=dev, dtype=dt)
    offs = torch.stack(torch.meshgrid(steps, steps, steps, indexing="ij"), dim=-1).reshape(1, n, n, n, 3)
    outs = [_sample(vol, cr / 2 ** i + offs).reshape(B, N, -1) for i, vol in enumerate(pyr)]
    return torch.cat(outs, dim=-1).permute(0, 2, 1).reshape(B, -1, H, W, D)


# ---------------------------------------------------------------------------------------------------------------
# the record: coordinates and ReLU decisions of the implementation under test
# ---------------------------------------------------------------------------------------------------------------
class Tape:
    """Recording (record=None): keeps coords1_i and act > 0 of every ReLU.  Consuming: hands the recorded coordinates
    out, replaces every ReLU by pre * mask and keeps, per ReLU, the share of elements where pre > 0 equals the mask."""

    def __init__(self, record=None):
        self.recording = record is None
        self.record = {"coords": [], "masks": {}} if record is None else record
        self.agreement = {}
        self.it = 0

    def coords(self, coords1):
        if self.recording:
            self.record["coords"].append(coords1.detach().cpu().clone())
            return coords1
        return self.record["coords"][self.it].to(device=coords1.device, dtype=coords1.dtype)

    def relu(self, name, pre):
        """A ReLU written out (library-form ops)."""
        if self.recording:
            return self.seen(name, F.relu(pre))
        mask = self.record["masks"][(self.it, name)].to(pre.device)
        self.agreement[(self.it, name)] = float(((pre.detach() > 0) == mask).double().mean())
        return pre * mask.to(pre.dtype)

    def seen(self, name, act):
        """The output of an op with the ReLU fused in (recording only)."""
        assert self.recording, "a fused ReLU cannot be teacher-forced"
        self.record["masks"][(self.it, name)] = (act.detach() > 0).cpu()
        return act


def upflow(flow, target_shape):
    """corr.py:211-253 out of place: trilinear, align_corners=True, channels 0..2 scaled by target / source size."""
    up = F.interpolate(flow, size=tuple(target_shape), mode="trilinear", align_corners=True)
    s = torch.ones(flow.shape[1], dtype=flow.dtype, device=flow.device)
    for c in range(min(3, flow.shape[1])):
        s[c] = target_shape[c] / flow.shape[2 + c]
    return up * s.view(1, -1, 1, 1, 1)


class LibraryOps:
    """The reference's ops as library calls in the dtype of their inputs, on any device: the restated lookup, F.conv3d,
    F.interpolate.  autocast=(device type, dtype) runs convc1 and the update block under torch.autocast, the
    reference's AMP arithmetic (raft_dvc.py:461-470); the correlation and the tail stay outside it, as there."""

    def __init__(self, num_levels=4, radius=4, autocast=None):
        self.num_levels, self.radius, self.autocast = num_levels, radius, autocast

    def _amp(self):
        if self.autocast is None:
            return torch.autocast("cpu", enabled=False)
        return torch.autocast(self.autocast[0], dtype=self.autocast[1])

    def corr(self, fmap1, fmap2):
        return pyramid(fmap1, fmap2, self.num_levels)

    def cor(self, tape, corr, coords1, p):
        x = lookup(corr, coords1, self.radius)
        with self._amp():
            return tape.relu("convc1", rl._conv(p, "encoder.convc1", x, 0))

    def gru_input(self, tape, p, context, flow, cor):
        """update.py:246-253 and the cat of update.py:338."""
        flo = tape.relu("convf1", rl._conv(p, "encoder.convf1", flow, 3))
        flo = tape.relu("convf2", rl._conv(p, "encoder.convf2", flo, 1))
        out = tape.relu("encoder.conv", rl._conv(p, "encoder.conv", torch.cat([cor, flo], dim=1), 1))
        return torch.cat([context, out, flow], dim=1)

    def heads(self, tape, p, net):
        outs = []
        for head in ("flow_head", "uncertainty_head"):
            if head + ".conv1.weight" in p:
                hid = tape.relu(head + ".conv1", rl._conv(p, head + ".conv1", net, 1))
                outs.append(rl._conv(p, head + ".conv2", hid, 1))
        return outs[0], (outs[1] if len(outs) > 1 else None)

    def block(self, tape, p, net, context, flow, cor):
        with self._amp():
            net = rl.sep_gru(p, net, self.gru_input(tape, p, context, flow, cor))
            delta, log_b = self.heads(tape, p, net)
        return net, delta, log_b

    def tail(self, coords1, delta, log_b, coords0, target_shape):
        coords1 = coords1 + delta
        up = upflow(coords1 - coords0, target_shape)
        return coords1, up, (None if log_b is None else upflow(log_b.to(up.dtype), target_shape))


class HipOps:
    """dvccorr's differentiable ops.  The update block is the hand-written chain of the public ops (which exposes
    every activation to the tape; update_block_ad's forward and backward are bit-identical to it) or, with
    fused_block=True, update_block_ad itself.  checkpoint=True wraps lookup_convc1 and the update block in
    torch.utils.checkpoint(..., use_reentrant=False): the reference's checkpoint_corr / checkpoint_updates."""

    def __init__(self, precision, block_cls, fused_block=False, checkpoint=False, num_levels=4, radius=4):
        assert fused_block or not checkpoint
        self.precision, self.block_cls, self.fused_block, self.checkpoint = precision, block_cls, fused_block, checkpoint
        self.num_levels, self.radius = num_levels, radius

    def corr(self, fmap1, fmap2):
        return self.block_cls(fmap1, fmap2, self.num_levels, self.radius, precision=self.precision)

    def _ckpt(self, fn, *args):
        if not self.checkpoint:
            return fn(*args)
        from torch.utils.checkpoint import checkpoint
        return checkpoint(fn, *args, use_reentrant=False)

    def cor(self, tape, corr, coords1, p):
        w, b = p["encoder.convc1.weight"], p["encoder.convc1.bias"]
        return tape.seen("convc1", self._ckpt(lambda c: corr.lookup_convc1(c, w, b), coords1))

    def block(self, tape, p, net, context, flow, cor):
        import dvccorr
        if self.fused_block:
            return self._ckpt(lambda n, c, r: dvccorr.update_block_ad(n, c, flow, p, cor=r, precision=self.precision),
                              net, context, cor)
        w = lambda l: (p[l + ".weight"], p[l + ".bias"])   # noqa: E731
        conv = lambda name, x, relu, x2=None: dvccorr.conv3x3x3_ad(   # noqa: E731
            x, *w(name), relu=relu, precision=self.precision, x2=x2)
        flo1 = tape.seen("convf1", dvccorr.conv7x7x7_flow_ad(flow, *w("encoder.convf1"), precision=self.precision))
        flo2 = tape.seen("convf2", conv("encoder.convf2", flo1, True))
        mot = tape.seen("encoder.conv", conv("encoder.conv", cor, True, flo2))
        inp = torch.cat([context, mot, flow], dim=1)
        net = dvccorr.sep_conv_gru_ad(net, inp, {n[4:]: t for n, t in p.items() if n.startswith("gru.")},
                                      precision=self.precision)
        delta = conv("flow_head.conv2", tape.seen("flow_head.conv1", conv("flow_head.conv1", net, True)), False)
        log_b = None
        if "uncertainty_head.conv1.weight" in p:
            hid = tape.seen("uncertainty_head.conv1", conv("uncertainty_head.conv1", net, True))
            log_b = conv("uncertainty_head.conv2", hid, False)
        return net, delta, log_b

    def tail(self, coords1, delta, log_b, coords0, target_shape):
        import dvccorr
        coords1, up = dvccorr.flow_step(coords1, delta, target_shape)
        return coords1, up, (None if log_b is None else dvccorr.upflow_3d(log_b, target_shape))


# ---------------------------------------------------------------------------------------------------------------
# the loop, its loss and the optimiser step
# ---------------------------------------------------------------------------------------------------------------
def grid(coords):
    B, _, H, W, D = coords.shape
    return torch.from_numpy(prng.identity_coords(B, H, W, D)).to(device=coords.device, dtype=coords.dtype)


def sequence_loss(ups, log_b_ups, gt, gamma):
    """loss.py:106-124: sum_i gamma^(n-i-1) mean over voxels of the end-point error |up_i - gt|_2.  (The reference's
    EPELoss at loss.py:47 sums the absolute differences of the three components instead of taking their 2-norm; the
    2-norm keeps the loss free of a fourth family of kinks, sign(up - gt), beside the ReLUs.  The weights, the mean and
    the sum over the iterations, which are what carries gradient across iterations, are the reference's.)  With an
    uncertainty head: plus, per iteration, a fixed pseudo-random linear functional of log_b_up with coefficients
    uniform in +-1 over the voxel count, so that both terms weigh alike."""
    n = len(ups)
    loss = 0.0
    for i, up in enumerate(ups):
        loss = loss + gamma ** (n - i - 1) * (up - gt).pow(2).sum(dim=1).sqrt().mean()
    for i, lb in enumerate(log_b_ups):
        c = torch.from_numpy(prng.uniform(LOG_B_SEED + i, tuple(lb.shape), -1.0, 1.0)).to(device=lb.device, dtype=lb.dtype)
        loss = loss + (c * lb).sum() / (lb.numel() // lb.shape[1])
    return loss


def train_loop(ops, f1, f2, params, net0, context, coords_init, gt, T_shape, iters, gamma=0.8, record=None):
    """raft_dvc.py:440-491 and the sequence loss.  record=None: the run records its detached coords1_i and the mask
    act > 0 of every ReLU (RELUS, per iteration).  A given record: the run looks up at those coordinates, replaces every
    ReLU by pre * mask and returns record["agreement"][(iteration, relu)], the share of pre > 0 == mask.
    Returns (loss, record)."""
    tape = Tape(record)
    corr = ops.corr(f1, f2)
    coords0 = grid(coords_init)
    coords1, net = coords_init, net0
    ups, log_b_ups = [], []
    for it in range(iters):
        tape.it = it
        coords1 = tape.coords(coords1.detach())
        cor = ops.cor(tape, corr, coords1, params)
        flow = coords1 - coords0
        net, delta, log_b = ops.block(tape, params, net, context, flow, cor)
        coords1, up, log_b_up = ops.tail(coords1, delta, log_b, coords0, T_shape)
        ups.append(up)
        if log_b_up is not None:
            log_b_ups.append(log_b_up)
    tape.record["agreement"] = tape.agreement
    return sequence_loss(ups, log_b_ups, gt, gamma), tape.record


def sgd_step(leaves, grads, rate=0.1):
    """In place, per tensor: w -= rate max|w| g / max|g|.  The largest change of every tensor is a tenth of its largest
    entry, so anything still packed from the old values is a 10 % error, not a rounding-size one."""
    with torch.no_grad():
        for k, w in leaves.items():
            g = grads[k].to(device=w.device, dtype=w.dtype)
            w.sub_(g * (rate * w.abs().max() / g.abs().max()))


# ---------------------------------------------------------------------------------------------------------------
# cases and the comparison
# ---------------------------------------------------------------------------------------------------------------
CASES = {
    # B, feature-map volume, target volume, iterations, the update_cases fixture whose block it uses
    "A": (1, (8, 10, 12), (61, 77, 93), 3, "upd_888"),     # levels 8.10.12, 4.5.6, 2.2.3, 1.1.1: partial tiles, a zero level
    "B": (2, (8, 8, 8), (64, 64, 64), 2, "upd_215"),       # two samples, the uncertainty head: _UpflowFn in the loop
}
_SEED = {"A": 9500, "B": 9600}


def case_inputs(name):
    """Float32 CPU tensors of a case, regenerated from the portable PRNG: leaves (fmap1, fmap2, net0, context and every
    parameter) and constants (coords_init, gt)."""
    import numpy as np
    import update_cases as uc
    B, vol, T, iters, block = CASES[name]
    s = _SEED[name]
    leaves = {"fmap1": prng.normal(s, (B, 32) + vol), "fmap2": prng.normal(s + 1, (B, 32) + vol),
              "net0": prng.uniform(s + 2, (B, 96) + vol, -1.0, 1.0),
              "context": np.maximum(prng.normal(s + 3, (B, 64) + vol), 0.0).astype(np.float32)}
    leaves = {k: torch.from_numpy(v) for k, v in leaves.items()}
    leaves.update({n: t.clone() for n, t in uc.params(block).items()})
    consts = {"coords_init": torch.from_numpy(prng.flow_coords(s + 4, B, *vol, 1.5)),
              "gt": torch.from_numpy(prng.uniform(s + 5, (B, 3) + T, -4.0, 4.0))}
    return leaves, consts, T, iters


INPUTS = ("fmap1", "fmap2", "net0", "context")


def run(ops, leaves, consts, T, iters, device, dtype, record=None, gamma=0.8, loss_scale=1.0):
    """One training step's forward and backward on copies of `leaves` that require grad (or, where `leaves` already
    holds leaf tensors on the device, on those).  Returns (loss, {name: gradient}, record)."""
    lv = {}
    for k, t in leaves.items():
        if t.requires_grad:
            t.grad = None
            lv[k] = t
        else:
            lv[k] = t.to(device=device, dtype=dtype).clone().requires_grad_(True)
    cs = {k: t.to(device=device, dtype=dtype) for k, t in consts.items()}
    params = {k: t for k, t in lv.items() if k not in INPUTS}
    loss, record = train_loop(ops, lv["fmap1"], lv["fmap2"], params, lv["net0"], lv["context"], cs["coords_init"],
                              cs["gt"], T, iters, gamma=gamma, record=record)
    (loss * loss_scale).backward()
    grads = {k: t.grad.detach() / loss_scale for k, t in lv.items()}
    return loss.detach(), grads, record


def errors(got, want):
    """Max-normalised error per tensor (update_cases.err), the loss included under "loss"."""
    import update_cases as uc
    (gl, gg), (wl, wg) = got, want
    assert set(gg) == set(wg)
    out = {k: uc.err(gg[k], wg[k]) for k in wg}
    out["loss"] = abs(float(gl) - float(wl)) / abs(float(wl))
    return out


def against_float64(ops, leaves, consts, T, iters, device, dtype, gamma=0.8, loss_scale=1.0, ref_gamma=0.8):
    """Run `ops` (recording) and the float64 CPU reference on its record.  Returns (errors per tensor and of the loss,
    mask agreement per (iteration, ReLU), (loss, grads) of the implementation, (loss, grads) of the reference)."""
    loss, grads, record = run(ops, leaves, consts, T, iters, device, dtype, gamma=gamma, loss_scale=loss_scale)
    cpu = {k: t.detach().cpu() for k, t in leaves.items()}
    rloss, rgrads, record = run(LibraryOps(), cpu, consts, T, iters, "cpu", torch.float64, record=record, gamma=ref_gamma)
    return errors((loss, grads), (rloss, rgrads)), record["agreement"], (loss, grads), (rloss, rgrads)
