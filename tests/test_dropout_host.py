"""Training-mode dropout without a GPU: the generator's three implementations agree (known answers, the
numpy restatement, the library's host function), the package generator's bookkeeping, the fp64 restatement against the
reference-made fixture tests/golden/G24_dropout.npz (where the masks go and the scale), and the refusals that are new.
The refusals that existed before (encoder, stand-alone attention modules, sequence and slice-learner families) have their
own tests and are not repeated."""
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_l2
import dropout_restatement as dr

G24 = os.path.join(GOLDEN, "G24_dropout.npz")


# ---------------------------------------------------------------------------------------------- the generator
def test_restatement_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        assert " ".join(f"{int(v):08x}" for v in dr.philox4x32_10(ctr, key)) == want
    assert dr.draw_words(1234, 0, 4).tolist() == [546353992, 3665621163, 1140953199, 3419031310]
    # batched evaluation equals one counter at a time
    both = dr.philox4x32_10([k[0] for k in kat], [k[1] for k in kat])
    assert [" ".join(f"{int(v):08x}" for v in row) for row in both] == [k[2] for k in kat]


THRESHES = (0, int(0.1 * 2 ** 32), 2 ** 31, 2 ** 32 - 1)


@pytest.mark.parametrize("seed,offset,first,count", [
    (1234, 0, 3, 41),                              # first not a multiple of 4
    (1234, 0, 0, 4), (1234, 7, 6, 1),
    (99, 2 ** 32 - 2, 0, 16),                      # carry into the high counter word
    (99, 2 ** 32 - 2, 5, 16),
    (0x9E3779B97F4A7C15, 12345, 2, 33),            # seed with high bits set
    (0xFFFFFFFFFFFFFFFF, 2 ** 64 - 2, 1, 18),      # the counter wraps at 2^64
])
def test_host_function_equals_restatement(seed, offset, first, count):
    from transformerbasednavierstokesolver_amd import ops
    for thresh in THRESHES:
        got = ops.dropout_keep_host(seed, offset, first, count, thresh).numpy()
        want = dr.keep_mask(seed, offset, count, thresh, first)
        assert np.array_equal(got, want), (thresh, got, want)
    assert ops.dropout_keep_host(seed, offset, first, count, 0).all()          # thresh 0 keeps everything


def test_keep_fraction():
    from transformerbasednavierstokesolver_amd import ops
    n = 2 ** 20
    for p in (0.1, 0.25, 0.5):
        thresh, scale = ops.dropout_constants(p)
        assert (thresh, scale) == dr.thresh_scale(p) and thresh == math.floor(p * 2 ** 32)
        assert scale == float(np.float32(1.0 / (1.0 - p)))
        sigma = math.sqrt(p * (1 - p) / n)
        for seed, offset in ((1234, 0), (0x9E3779B97F4A7C15, 2 ** 32 - 7)):
            frac = float(ops.dropout_keep_host(seed, offset, 0, n, thresh).double().mean())
            assert abs(frac - (1 - p)) <= 4 * sigma, (p, seed, (frac - (1 - p)) / sigma)


def test_package_generator():
    from transformerbasednavierstokesolver_amd import ops
    ops.dropout_manual_seed(77)
    assert ops.dropout_state() == (77, 0)
    assert ops.dropout_reserve(5) == (77, 0) and ops.dropout_state() == (77, 2)          # ceil(5 / 4) counters
    assert ops.dropout_reserve(8) == (77, 2) and ops.dropout_state() == (77, 4)
    assert ops.dropout_reserve(0) == (77, 4) and ops.dropout_state() == (77, 4)
    # consecutive draws share no counter: the words of the two draws are the words of one longer draw, in order
    a, b = dr.draw_words(77, 0, 5), dr.draw_words(77, 2, 8)
    whole = dr.draw_words(77, 0, 16)
    assert np.array_equal(a, whole[:5]) and np.array_equal(b, whole[8:16])
    # without an explicit seed the generator follows torch's, and re-latches when that changes
    torch.manual_seed(4321)
    assert ops.dropout_state() == (4321, 0)
    ops.dropout_reserve(100)
    assert ops.dropout_state() == (4321, 25)
    torch.manual_seed(4322)
    assert ops.dropout_state() == (4322, 0)
    ops.dropout_manual_seed(2 ** 64 + 5)            # seeds are taken modulo 2^64
    assert ops.dropout_state() == (5, 0)


def test_token_case_masks_leave_enough_rows():
    """The seeds of the GPU token-attention cases: at most one row in eight keeps nothing (checked here, on the CPU)."""
    for case in dr.TOKEN_CASES:
        for p in dr.TOKEN_PS:
            mask, rows = dr.token_mask(*case, p)
            assert (~rows).sum() * 8 <= rows.size, (case, p, int((~rows).sum()))
            assert abs(mask.mean() - (1 - p)) < 0.1


# ---------------------------------------------------------------------------------------------- where the masks go
@pytest.mark.parametrize("tag", ["2d", "irregular"])
def test_restatement_reproduces_the_reference(tag):
    """fp64 restatement with the fixture's masks against the reference's outputs and gradients (made by
    tools/make_golden_dropout.py with the reference's nn.Dropout members replaced by these masks)."""
    g = np.load(G24)
    pre = tag + "."
    cfg = json.loads(str(g[pre + "config"]))
    sd = {k[len(pre) + 3:]: torch.from_numpy(g[k]).double().requires_grad_(True) for k in g.files if k.startswith(pre + "sd.")}
    x, fx, gy = (torch.from_numpy(g[pre + k]).double() for k in ("x", "fx", "gy"))
    B, N = x.shape[:2]
    thresh, scale, seed = int(g[pre + "thresh"]), float(g[pre + "scale"]), int(g[pre + "seed"])
    assert (thresh, scale) == dr.thresh_scale(float(g[pre + "p"]))
    masks, _ = dr.layer_masks(seed, 0, thresh, cfg["n_layers"], B, cfg["n_head"], cfg["slice_num"], N, cfg["n_hidden"])
    for i, (ma, mo) in enumerate(masks):            # the fixture's masks are the draws of the contract
        assert np.array_equal(ma.numpy().astype(np.uint8), g[f"{pre}mask.{i}.attn"])
        assert np.array_equal(mo.numpy().astype(np.uint8), g[f"{pre}mask.{i}.out"])
    out = dr.model_forward(sd, x, fx, tag, (cfg["H"], cfg["W"]) if tag == "2d" else None, cfg, masks, scale)
    assert rel_l2(out, g[pre + "pred.f64"]) <= 1e-12
    assert rel_l2(g[pre + "pred.f32"], g[pre + "pred.f64"]) <= 2e-5
    out.backward(gy)
    ngrad = 0
    for k, t in sd.items():
        if pre + "grad.f64." + k in g.files:
            assert rel_l2(t.grad, g[pre + "grad.f64." + k]) <= 1e-12, k
            ngrad += 1
        else:
            assert t.grad is None or not t.grad.any(), k
    assert ngrad >= len(sd) - 1
    # the masks matter: without them the output is far away
    ones = [(torch.ones_like(a), torch.ones_like(b)) for a, b in masks]
    plain = dr.model_forward(sd, x, fx, tag, (cfg["H"], cfg["W"]) if tag == "2d" else None, cfg, ones, 1.0)
    assert rel_l2(plain, g[pre + "pred.f64"]) > 1e-3


# ---------------------------------------------------------------------------------------------- refusals
def _tiny_2d(dropout):
    from transformerbasednavierstokesolver_amd.model.Transolver_Structured_Mesh_2D import Model
    return Model(space_dim=2, n_layers=2, n_hidden=32, dropout=dropout, n_head=4, fun_dim=3, out_dim=1, slice_num=8, H=6, W=5)


def test_graphed_steps_refuse_training_dropout_without_a_gpu():
    from transformerbasednavierstokesolver_amd import harness
    m = _tiny_2d(0.1).train()
    assert harness.training_dropout(m) == pytest.approx(0.1)
    with pytest.raises(NotImplementedError, match="dropout"):
        harness.GraphedTrainStep(m, None, None, None, None, None)
    with pytest.raises(NotImplementedError, match="dropout"):
        harness.GraphedCallStep(m, None, None, (), None)
    # in eval mode, and at p = 0, this check lets the model pass (the next one asks for the fused optimizer)
    assert harness.training_dropout(m.eval()) == 0.0 and harness.training_dropout(_tiny_2d(0.0).train()) == 0.0
    with pytest.raises(TypeError):
        harness.GraphedTrainStep(m.eval(), None, None, None, None, None)


def test_p_one_is_refused():
    from transformerbasednavierstokesolver_amd import ops
    with pytest.raises(ValueError):
        ops.dropout_constants(1.0)
    m = _tiny_2d(1.0).train()
    with pytest.raises(ValueError):
        m.blocks[0](torch.zeros(1, 30, 32))
    assert ops.dropout_constants(0.0) == (0, 1.0)


def test_bf16_storage_with_dropout_is_refused():
    m = _tiny_2d(0.1).train().set_engine("bf16s")
    with pytest.raises(NotImplementedError, match="fp32 storage"):
        m.blocks[0](torch.zeros(1, 30, 32))
    with pytest.raises(NotImplementedError, match="fp32 storage"):
        m.set_engine("split").blocks[0](torch.zeros(1, 30, 32, dtype=torch.bfloat16))


def test_checkpointed_blocks_refuse_training_dropout():
    """torch.utils.checkpoint runs a block again in the backward; that run would reserve new draws."""
    from transformerbasednavierstokesolver_amd.model.Transolver_Structured_Mesh_3D import Model
    m = Model(space_dim=3, n_layers=2, n_hidden=32, dropout=0.1, n_head=4, fun_dim=1, out_dim=1, slice_num=8, H=4, W=5, D=3).train()
    m.use_checkpoint = True
    with pytest.raises(NotImplementedError, match="use_checkpoint"):
        m._run_blocks(torch.zeros(1, 60, 32))


def test_blocks_declare_what_they_serve():
    from transformerbasednavierstokesolver_amd.model import (Transolver_Irregular_Mesh, Transolver_Structured_Mesh_2D,
                                                             Transolver_Structured_Mesh_3D, Transolver_Structured_Mesh2D_Encoder)
    from transformerbasednavierstokesolver_amd.model._core import BlockBase
    assert not BlockBase.serves_dropout and not Transolver_Structured_Mesh2D_Encoder.Transolver_Encoder_block.serves_dropout
    for mod in (Transolver_Irregular_Mesh, Transolver_Structured_Mesh_2D, Transolver_Structured_Mesh_3D):
        assert mod.Transolver_block.serves_dropout
