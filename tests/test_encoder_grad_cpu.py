"""CPU: the float64 restatement with a ReLU tape (tests/encoder_grad.py) against tests/raftdvc_encoder.py's module and
the reference's fixture, and what dvccorr.encoder_ad promises without a GPU: size functions, argument validation, fake
implementations, the refusal of a volume that requires grad."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import encoder_grad as eg
import prng
import raftdvc_encoder as renc
from conftest import load_golden


def _module_and_sd(kind, seed0=300):
    m = renc.Encoder(kind, output_dim=128).double().eval()
    renc.set_params(m, seed0)
    return m, {n: p for n, p in m.state_dict(keep_vars=True).items()}


def _x(shape, seed=77):
    return torch.from_numpy(prng.uniform(seed, shape, -1.0, 1.0)).double()


def test_restatement_equals_module_forward_and_gradients():
    m, sd = _module_and_sd("1/8")
    x = _x((2, 1, 13, 18, 10))
    G = _x((2, 128, 2, 3, 2), 78)
    (m(x) * G).sum().backward()
    ref = {n: p.grad.clone() for n, p in m.named_parameters()}
    lv = eg.leaves(sd, torch.float64, "cpu")
    y = eg.encoder(x, lv, eg.STRIDES["1/8"], "instance")
    assert torch.allclose(y, m(x).detach(), rtol=0, atol=1e-12)
    (y * G).sum().backward()
    for n, g in ref.items():
        assert float((lv[n].grad - g).abs().max()) <= 1e-12 * max(1.0, float(g.abs().max())), n


def test_restatement_reproduces_fixture():
    g = load_golden("encoder_1_8.npz")
    m, sd = _module_and_sd("1/8", int(g["seed0"][0]))
    x = torch.from_numpy(prng.uniform(int(g["in_seed"][0]), tuple(int(v) for v in g["in_shape"])))
    y = eg.encoder(x.double(), {n: p.detach() for n, p in sd.items()}, eg.STRIDES["1/8"], "instance")
    ref = torch.from_numpy(np.asarray(g["out"])).double()
    assert float((y - ref).abs().max() / ref.abs().max()) <= 1e-5


def test_consuming_own_record_gives_same_gradients():
    sd = eg.make_weights(eg.STRIDES["1/1"], 128, 4500)
    x = _x((1, 1, 9, 6, 17))
    G = _x((1, 128, 9, 6, 17), 79)
    a = eg.leaves(sd, torch.float64, "cpu")
    rec = eg.Tape()
    (eg.encoder(x, a, eg.STRIDES["1/1"], "instance", rec) * G).sum().backward()
    assert len(rec.masks) == 1 + 3 * 6
    b = eg.leaves(sd, torch.float64, "cpu")
    con = eg.Tape(rec.masks)
    (eg.encoder(x, b, eg.STRIDES["1/1"], "instance", con) * G).sum().backward()
    assert set(con.agree.values()) == {1.0}
    for n in a:
        assert torch.allclose(a[n].grad, b[n].grad, rtol=1e-12, atol=1e-14), n


@pytest.mark.parametrize("case", ("A", "B", "C"))
def test_float32_masks_agree_with_float64(case):
    """The seeds of the GPU test: a float32 CPU run's ReLU masks agree with float64's within the GPU test's cap."""
    import test_gpu_encoder_grad as tg
    c = tg.CASES[case]
    out = {}
    for dt in (torch.float64, torch.float32):
        tape = eg.Tape()
        tg._restated(case, {n: w.to(dt) for n, w in tg._weights(case).items()}, [x.to(dt) for x in tg._inputs(case)], tape)
        out[dt] = tape.masks
    for n, m in out[torch.float64].items():
        assert float((m == out[torch.float32][n]).double().mean()) >= tg.AGREE_MIN, (case, n)
    assert c["norm"] in ("instance", "none")


def test_size_functions_and_validation():
    from dvccorr import _lib, ops
    L = _lib.lib()
    assert L.dvc_enc_grad_partials_bytes(24, 2, 9, 30, 17) == 2 * 24 * 2 * 3 * 8
    assert L.dvc_enc_grad_partials_bytes(0, 2, 9, 30, 17) == 0
    nk, per, nslab = ops.enc_wgrad_slabs(27, 2, 8, 8, 2, (5, 6, 17))
    assert L.dvc_enc_wgrad_workspace_bytes(27, 2, 8, 8, 2, 5, 6, 17) == nslab * 8 * 8 * 27 * 4
    assert L.dvc_enc_wgrad_workspace_bytes(1, 1, 96, 160, 2, 5, 6, 17) == ops.enc_wgrad_slabs(1, 1, 96, 160, 2, (5, 6, 17))[2] \
        * 96 * 160 * 4
    assert L.dvc_enc_wgrad_workspace_bytes(27, 1, 12, 8, 2, 5, 6, 17) == 0       # cin no multiple of 8
    assert L.dvc_enc_wgrad_workspace_bytes(1, 1, 96, 176, 2, 5, 6, 17) == 0      # wider than 160
    assert L.dvc_enc_wgrad_workspace_bytes(343, 1, 1, 32, 2, 5, 6, 17) == 0      # the stem has its own entry
    assert L.dvc_enc_stem_wgrad_workspace_bytes(2, 2, 9, 6, 17) > 0
    assert L.dvc_enc_stem_wgrad_workspace_bytes(3, 2, 9, 6, 17) == 0
    # the dgrad pack of a layer is the forward pack of the swapped layer; K up to 160 here
    assert L.dvc_enc_dgrad_packed_bytes(27, 16, 24, 0) == L.dvc_enc_conv_packed_bytes(27, 24, 16, 0)
    assert L.dvc_enc_dgrad_packed_bytes(1, 96, 160, 2) > 0 and L.dvc_enc_conv_packed_bytes(1, 160, 96, 2) == 0
    assert L.dvc_enc_dgrad_packed_bytes(1, 96, 161, 2) == 0
    assert L.dvc_enc_norm_grad(None, None, None, 0, None, None, None, 8, 1, 4, 4, 4, None) == _lib.DVC_ERR_INVALID
    assert L.dvc_enc_wgrad(None, None, 0, None, None, None, 27, 1, 8, 8, 1, 4, 4, 4, 0, None) == _lib.DVC_ERR_INVALID
    assert L.dvc_enc_dgrad(None, None, None, 27, 1, 8, 8, 1, 4, 4, 4, 0, None) == _lib.DVC_ERR_INVALID
    assert ops.enc_grad_covers(1, 96, 160) and not ops.enc_grad_covers(27, 12, 8) and not ops.enc_grad_covers(1, 168, 8)


def test_operators_have_fake_implementations():
    import dvccorr  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    sd = eg.make_weights(eg.STRIDES["1/8"], 160, 1, dtype=torch.float32)
    with FakeTensorMode():
        O = torch.ops.dvccorr
        x = torch.empty(2, 1, 13, 18, 10)
        names = __import__("dvccorr").Encoder(sd, "1/8").names   # the operator's weight order
        outs = O.encoder_ad(x, [torch.empty(sd[n].shape) for n in names], [2, 1, 2, 2], True, 96, 1e-5, 0)
        assert tuple(outs[0].shape) == (2, 96, 2, 3, 2) and tuple(outs[1].shape) == (2, 64, 2, 3, 2)
        assert len(outs) == 2 + 2 * 21 + 6   # 21 raw outputs with their tables, six block outputs
        g = torch.empty(2, 8, 3, 3, 9)
        assert tuple(O.enc_wgrad(torch.empty(2, 8, 5, 6, 17), None, 1, g, 27, 2, 0).shape) == (8, 8, 3, 3, 3)
        assert tuple(O.enc_dgrad(g, torch.empty(10), 27, 2, 8, [5, 6, 17], 0).shape) == (2, 8, 5, 6, 17)
        gx, db = O.enc_norm_grad(g, g, None, True, True, False)
        assert gx.shape == g.shape and db.numel() == 0
        assert O.enc_grad_add(g, None, g).shape == g.shape
        assert tuple(O.enc_split_grad(g, None, g, g).shape) == (2, 16, 3, 3, 9)
        assert O.enc_pack_dgrad(torch.empty(24, 16, 3, 3, 3), 0).numel() * 4 == \
            __import__("dvccorr")._lib.lib().dvc_enc_dgrad_packed_bytes(27, 16, 24, 0)


def test_volume_that_requires_grad_is_refused():
    import dvccorr
    sd = eg.make_weights(eg.STRIDES["1/8"], 128, 1, dtype=torch.float32)
    x = torch.zeros(1, 1, 8, 8, 8, requires_grad=True)
    with pytest.raises(NotImplementedError, match="volume"):
        dvccorr.encoder_ad(x, sd)
    with pytest.raises(NotImplementedError, match="volume"):
        dvccorr.encoder_ad([x.detach(), x], sd)
    with pytest.raises(NotImplementedError, match="volume"):
        dvccorr.context_encoder_ad(x, eg.make_weights(eg.STRIDES["1/8"], 160, 1, "encoder.", torch.float32))
