"""Structured 3-D mesh family without a GPU: the module's interface against the reference (tests/golden/G8_structured3d.npz,
written by tools/make_golden_3d.py), the new C ABI symbols and the host-side refusals."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

G8 = os.path.join(GOLDEN, "G8_structured3d.npz")


@pytest.fixture(scope="module")
def g8():
    return np.load(G8)


def regenerate(g8, pre):
    """The case's state_dict: keys / shapes from the fixture, values from the seeded generator (checked by their sums)."""
    from transformerbasednavierstokesolver_amd import synth
    keys = [str(k) for k in g8[pre + "keys"]]
    shapes = json.loads(str(g8[pre + "shapes"]))
    sd = synth.synth_state_dict_from_spec(list(zip(keys, shapes)), seed=int(g8[pre + "seed"]), wild_temperature=True)
    sums = np.array([np.sum(sd[k], dtype=np.float64) for k in keys])
    np.testing.assert_allclose(sums, g8[pre + "sums"], rtol=1e-12, atol=1e-12)
    return {k: torch.from_numpy(v) for k, v in sd.items()}


def tiny_model(g8, variant):
    from transformerbasednavierstokesolver_amd.model.Transolver_Structured_Mesh_3D import Model
    cfg = json.loads(str(g8[f"tiny_{variant}.config"]))
    torch.manual_seed(0)
    return Model(**cfg), cfg


def test_constructor_signature_and_name_match_reference(g8):
    from transformerbasednavierstokesolver_amd.model.Transolver_Structured_Mesh_3D import Model
    ref = [tuple(p) for p in json.loads(str(g8["signature"]))]
    ours = [(k, p.default) for k, p in inspect.signature(Model.__init__).parameters.items() if k != "self"]
    assert ours == ref
    m = Model(n_layers=1, n_hidden=32, n_head=4, H=2, W=3, D=4)
    assert m.__name__ == str(g8["name"]) == "Transolver_3D"
    assert m.use_checkpoint is False


@pytest.mark.parametrize("variant", ["up", "nofx", "time"])
def test_state_dict_keys_shapes_and_strict_load(g8, variant):
    m, _ = tiny_model(g8, variant)
    pre = f"tiny_{variant}."
    sd = regenerate(g8, pre)
    ours = m.state_dict()
    assert list(ours) == [str(k) for k in g8[pre + "keys"]]
    assert [list(v.shape) for v in ours.values()] == json.loads(str(g8[pre + "shapes"]))
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert tuple(m.blocks[0].Attn.in_project_x.weight.shape) == (32, 32, 3, 3, 3)


def test_attention_module_state_dict_matches_reference(g8):
    from transformerbasednavierstokesolver_amd.model.Physics_Attention import Physics_Attention_Structured_Mesh_3D
    for case in ("8x8x8", "1x6x5", "3x1x7"):
        pre = f"attn_{case}."
        H, W, D, C, heads, M, _ = (int(v) for v in g8[pre + "geom"])
        a = Physics_Attention_Structured_Mesh_3D(C, heads=heads, dim_head=C // heads, slice_num=M, H=H, W=W, D=D)
        assert list(a.state_dict()) == [str(k) for k in g8[pre + "keys"]]
        a.load_state_dict(regenerate(g8, pre), strict=True)
        assert (a.H, a.W, a.D) == (H, W, D) and a.mesh_w == (W, D)


def test_get_grid_matches_reference_pos(g8):
    from transformerbasednavierstokesolver_amd.model.Transolver_Structured_Mesh_3D import Model
    m = Model(n_layers=1, n_hidden=32, n_head=4, unified_pos=True, ref=4, H=4, W=5, D=3)
    want = torch.from_numpy(g8["pos_4x5x3_ref4"])
    got = m.pos
    assert got.dtype == torch.float32 and got.shape == want.shape == (1, 4, 5, 3, 64)
    assert "pos" not in m.state_dict()
    ulp = torch.finfo(torch.float32).eps * want.abs().clamp_min(torch.finfo(torch.float32).tiny)
    assert bool(((got - want).abs() <= 2 * ulp).all()), float(((got - want).abs() / ulp).max())
    assert m.preprocess.linear_pre[0].in_features == 1 + 64


def test_c_abi_3d_symbols_exported_and_bound():
    import ctypes
    from transformerbasednavierstokesolver_amd import _lib
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("pa2d_conv3x3x3x2_workspace", "pa2d_conv3x3x3x2_fwd_workspace", "pa2d_conv3x3x3x2_pack_bytes",
                 "pa2d_conv3x3x3x2_pack", "pa2d_conv3x3x3x2_fwd", "pa2d_conv3x3x3x2_bwd"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
    for C in (16, 32, 256):
        pb = lib.pa2d_conv3x3x3x2_pack_bytes(C)
        assert pb == 3 * 27 * C * C * 4
        for engine in (0, 1, 2):
            assert lib.pa2d_conv3x3x3x2_workspace(0, 4, 5, 3, C, engine) >= pb
            assert lib.pa2d_conv3x3x3x2_fwd_workspace(0, 4, 5, 3, C, engine) >= pb
            assert lib.pa2d_conv3x3x3x2_workspace(2, 32, 32, 32, C, engine) >= pb
    # host-side argument checks: refused before any launch (null pointers are never touched)
    assert lib.pa2d_conv3x3x3x2_fwd(0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2, 2, 2, 24, 1, 0, 0, 0) == 1002     # C % 16
    assert lib.pa2d_conv3x3x3x2_fwd(0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2, 0, 2, 32, 1, 0, 0, 0) == 1001     # W = 0
    assert lib.pa2d_conv3x3x3x2_fwd(0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2, 2, 2, 32, 7, 0, 0, 0) == 1001     # engine
    assert lib.pa2d_conv3x3x3x2_fwd(0, 0, 0, 0, 0, 0, 0, 0, 0, 1024, 1024, 1024, 2, 32, 1, 0, 0, 0) == 1002  # rows > int
    assert lib.pa2d_conv3x3x3x2_fwd(0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2, 2, 2, 32, 1, 0, 0, 0) == 1003     # workspace
    assert lib.pa2d_conv3x3x3x2_fwd(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 2, 2, 32, 1, 0, 0, 0) == 0        # B = 0: no-op
    assert lib.pa2d_conv3x3x3x2_bwd(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2, 2, 2, 32, 0, 1, 0, 0, 0) == 1003


def test_bf16_storage_refused_on_3d_model():
    from transformerbasednavierstokesolver_amd.model.Transolver_Structured_Mesh_3D import Model
    m = Model(n_layers=1, n_hidden=32, n_head=4, H=2, W=3, D=4)
    with pytest.raises(NotImplementedError):
        m.set_engine("bf16s")
    m.set_engine("split")                # the fp32-storage engines are accepted
    from transformerbasednavierstokesolver_amd import ops
    m.engine = ops.ENGINE_BF16S          # set behind set_engine's back: refused when the blocks run
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 24, 1), torch.zeros(1, 24, 1))


def test_registry_still_refuses_3d_and_points_at_the_module():
    import types
    from transformerbasednavierstokesolver_amd.model_dict import get_model
    with pytest.raises(KeyError, match="model.Transolver_Structured_Mesh_3D"):
        get_model(types.SimpleNamespace(model="Transolver_Structured_Mesh_3D"))


def test_mesh_extent_and_unsupported_settings():
    from transformerbasednavierstokesolver_amd import functional as Fn
    from transformerbasednavierstokesolver_amd.model.Physics_Attention import Physics_Attention_Structured_Mesh_3D
    assert Fn.mesh_extent(7) == (7, None) and Fn.mesh_extent((7, 3)) == (7, 3)
    with pytest.raises(NotImplementedError):
        Physics_Attention_Structured_Mesh_3D(32, heads=4, dim_head=8, kernel=5)
    with pytest.raises(NotImplementedError):
        Physics_Attention_Structured_Mesh_3D(32, heads=4, dim_head=16)
    a = Physics_Attention_Structured_Mesh_3D(32, heads=4, dim_head=8, dropout=0.1, H=2, W=2, D=2).train()
    with pytest.raises(NotImplementedError):
        a(torch.zeros(1, 8, 32))
