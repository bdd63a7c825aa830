"""Host-side contract of the fused block tail (include/pa2d.h: pa2d_block_tail_*): the symbols and their
arity, the shapes the library takes and refuses, the LDS budget, refusals before any launch, and the routing of
`set_fused_tail` in the models (which calls a flagged model makes, recorded through stand-ins of the `ops` functions).
No GPU is needed: every library call here returns on the host."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
from transformerbasednavierstokesolver_amd import _lib, ops
from transformerbasednavierstokesolver_amd.model import Transolver_Irregular_Mesh as irregular
from transformerbasednavierstokesolver_amd.model import Transolver_Structured_Mesh_2D as structured
from transformerbasednavierstokesolver_amd.model import Transolver_Structured_Mesh_3D as structured3d

UNSUPPORTED = 1002
NEW = {"pa2d_block_tail_supported": 7, "pa2d_block_tail_lds_bytes": 7, "pa2d_block_tail_image_bytes": 2,
       "pa2d_block_tail_weight_image": 8, "pa2d_block_tail_workspace": 2, "pa2d_block_tail_fwd": 39}
REQUIRED = [(C, C // D, D, M, r * C) for C in (64, 128, 256) for D in (8, 16, 32, 64) for M in (1, 12, 32, 64, 96, 128)
            for r in (1, 2, 4)]


def test_symbols_are_declared_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pa2d.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in NEW.items():
        m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
        assert m, f"{name} is not declared in include/pa2d.h"
        assert len(m.group(1).split(",")) == nargs, (name, len(m.group(1).split(",")))
        assert hasattr(raw, name), f"{name} is not exported"
        assert len(_lib.SIGNATURES[name][1]) == nargs, (name, len(_lib.SIGNATURES[name][1]))
    _lib.load()


def test_supported_shapes_and_lds_budget():
    lib = _lib.load()
    for C, heads, D, M, hidden in REQUIRED:
        for act in range(8):
            assert lib.pa2d_block_tail_supported(C, heads, D, M, hidden, act, 1) == 1, (C, heads, D, M, hidden, act)
        lds = lib.pa2d_block_tail_lds_bytes(C, heads, D, M, hidden, 1, 1)
        assert 0 < lds <= 160 * 1024, (C, heads, D, M, hidden, lds)
    # outside the kernel: D = 12, M = 129, hidden = 3 C + 4; an activation id or flag bit it does not know
    assert lib.pa2d_block_tail_supported(96, 8, 12, 64, 96, 1, 1) == 0
    assert lib.pa2d_block_tail_supported(256, 8, 32, 129, 256, 1, 1) == 0
    assert lib.pa2d_block_tail_supported(256, 8, 32, 64, 3 * 256 + 4, 1, 1) == 0
    assert lib.pa2d_block_tail_supported(256, 8, 32, 64, 256, 8, 1) == 0
    assert lib.pa2d_block_tail_supported(256, 8, 32, 64, 256, 1 | 0x100, 1) == 0
    assert lib.pa2d_block_tail_supported(256, 4, 32, 64, 256, 1, 1) == 0          # heads * D != C
    assert lib.pa2d_block_tail_lds_bytes(96, 8, 12, 64, 96, 1, 1) == 0
    # arithmetic of one engine is never run under another's id: the exact and the one-term engines have no fused tail
    for engine in (0, 2, 3, -1):
        assert lib.pa2d_block_tail_supported(256, 8, 32, 64, 256, 1, engine) == 0, engine
    assert ops.block_tail_supported(256, 8, 32, 64, 1024, "gelu", "split")
    assert not ops.block_tail_supported(256, 8, 32, 64, 1024, "gelu", "bf16s")
    assert not ops.block_tail_supported(256, 8, 32, 64, 1024, "gelu", "f32")


def _fwd_null(lib, B, N, heads, D, M, hidden, act, engine, ldx=None):
    C = heads * D
    return lib.pa2d_block_tail_fwd(0, 2 * C if ldx is None else ldx, 0, 0, 0, 0, 0, C, *(0,) * 18, 0, 0, B, N, heads, D, M,
                                   hidden, act, 1, engine, 1e-5, 0)


def test_fwd_refuses_before_any_launch():
    """NULL pointers and stream 0 throughout: only inputs that must return before a pointer is looked at."""
    lib = _lib.load()
    for heads, D, M, hidden, engine in ((8, 12, 64, 96, 1), (8, 32, 129, 256, 1), (8, 32, 64, 3 * 256 + 4, 1), (8, 32, 64, 256, 0),
                                        (8, 32, 64, 256, 2)):
        assert lib.pa2d_block_tail_supported(heads * D, heads, D, M, hidden, 1, engine) == 0
        assert _fwd_null(lib, 2, 64, heads, D, M, hidden, 1, engine) == UNSUPPORTED, (heads, D, M, hidden, engine)
    # an operand past 4 GiB: x_mid rows of pitch 2 C (2^22 rows x 512 floats = 8 GiB), then the hidden layer's debug rows
    assert lib.pa2d_block_tail_supported(256, 8, 32, 64, 256, 1, 1) == 1
    assert _fwd_null(lib, 64, 1 << 16, 8, 32, 64, 256, 1, 1) == UNSUPPORTED
    assert _fwd_null(lib, 1, 1 << 20, 8, 32, 64, 1024, 1, 1, ldx=256) == UNSUPPORTED
    assert _fwd_null(lib, 0, 64, 8, 32, 64, 256, 1, 1) == 0                      # B = 0 is a no-op
    # the image helper: shape and engine before the buffer
    assert lib.pa2d_block_tail_weight_image(0, 256, 0, 0, 256, 256, 0, 0) == UNSUPPORTED
    assert lib.pa2d_block_tail_weight_image(0, 250, 0, 0, 256, 250, 1, 0) == UNSUPPORTED
    assert lib.pa2d_block_tail_image_bytes(256, 1024) == 256 * 1024 * 6
    assert lib.pa2d_block_tail_workspace(256, 1024) == 6 * (256 * 256 + 2 * 256 * 1024)


def _models():
    yield structured.Model(space_dim=2, n_layers=2, n_hidden=64, n_head=4, fun_dim=3, out_dim=1, slice_num=8, H=5, W=7), 35
    yield irregular.Model(space_dim=2, n_layers=2, n_hidden=64, n_head=4, fun_dim=3, out_dim=1, slice_num=8), 33
    yield structured3d.Model(space_dim=3, n_layers=2, n_hidden=64, n_head=4, fun_dim=3, out_dim=1, slice_num=8, H=2, W=3,
                             D=4), 24


def test_set_fused_tail_returns_the_model_and_reaches_every_block():
    for model, _ in _models():
        assert model.fused_tail is False
        assert all(b.fused_tail is False for b in model.blocks)
        assert model.set_fused_tail(True) is model
        assert all(b.fused_tail is True for b in model.blocks) and model.fused_tail is True
        assert model.set_fused_tail(False) is model
        assert not any(b.fused_tail for b in model.blocks)
    from transformerbasednavierstokesolver_amd.model.SOL_Transolver_Structured_Mesh_2D import SOL_Transolver_Structured_Mesh_2D
    sol = SOL_Transolver_Structured_Mesh_2D(space_dim=2, n_layers=2, n_hidden=64, n_head=4, fun_dim=3, slice_num=8, H=5, W=7)
    assert sol.set_fused_tail(True) is sol and all(b.fused_tail for b in sol.transolver_model.blocks)


def _record(monkeypatch):
    """Stand-ins for every `ops` function a model forward reaches: they record their name and return zeros of the
    right shape and storage type (CPU tensors; nothing native runs)."""
    calls = []
    z = lambda *shape, like: torch.zeros(*shape, dtype=like.dtype)

    def linear_fwd(x2d, w, bias=None, res=None, act=None, want_pre=False, engine=None, save_derivative=False):
        y = z(x2d.shape[0], w.shape[0], like=x2d)
        return y, (torch.zeros_like(y) if want_pre else None)

    def layernorm_fwd(x2d, gamma, beta, eps=1e-5):
        return torch.zeros_like(x2d), torch.zeros(x2d.shape[0]), torch.zeros(x2d.shape[0])

    def conv(xn, *a, **k):
        return z(xn.shape[0], xn.shape[1], 2 * xn.shape[2], like=xn)

    def slice_scatter(xm, ldx, xo, v, ldv, vo, ws_w, bs, temperature, B, N, heads, D, M, **k):
        return torch.zeros(B * heads, 1, M, D), torch.zeros(B * heads, 1, M)

    def token_attn_fwd(spart, npart, wq, wk, wv):
        BH, _, M, D = spart.shape
        return torch.zeros(BH, M, D), torch.zeros(BH, M), torch.zeros(BH, M, D)

    def deslice_fwd(xm, ldx, xo, o, ws_w, bs, temperature, B, N, heads, D, M, **k):
        return z(B, N, heads * D, like=xm)

    def head_fwd(x2d, w, b):
        return torch.zeros(x2d.shape[0], w.shape[0])

    def block_tail_fwd(xm, ldx, xo, o, ws_w, bs, temperature, fx2d, wo, bo, g2, be2, w1, b1, w2, b2, gn, bn, *a, **k):
        return torch.zeros_like(fx2d), (None if gn is None else torch.zeros_like(fx2d)), None

    fakes = dict(linear_fwd=linear_fwd, layernorm_fwd=layernorm_fwd, conv3x3x2_fwd=conv, conv3x3x3x2_fwd=conv,
                 slice_scatter=slice_scatter, token_attn_fwd=token_attn_fwd, deslice_fwd=deslice_fwd, head_fwd=head_fwd,
                 block_tail_fwd=block_tail_fwd, conv_planes_mask=lambda *a, **k: 0)
    for name, fn in fakes.items():
        def spy(*a, _f=fn, _n=name, **k):
            if _n != "conv_planes_mask":
                calls.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, spy)
    return calls


def _forward(model, N):
    return model(torch.zeros(3, N, model.space_dim), fx=torch.zeros(3, N, 3))


OLD_BLOCK = ["layernorm_fwd", "CONV", "slice_scatter", "token_attn_fwd", "deslice_fwd", "linear_fwd", "layernorm_fwd",
             "linear_fwd", "linear_fwd"]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_flagged_model_routes(monkeypatch, which):
    model, N = list(_models())[which]
    conv = ["conv3x3x2_fwd", "linear_fwd", "conv3x3x3x2_fwd"][which]
    old = ["linear_fwd"] * 2 + [conv if c == "CONV" else c for c in OLD_BLOCK] * 2 + ["layernorm_fwd", "head_fwd"]
    new = ["linear_fwd"] * 2 + ["layernorm_fwd"] + [conv, "slice_scatter", "token_attn_fwd", "block_tail_fwd"] * 2 + ["head_fwd"]
    calls = _record(monkeypatch)
    model.eval().set_engine("split")

    def run(grad=False, expect=None):
        del calls[:]
        with (torch.enable_grad() if grad else torch.no_grad()):
            out = _forward(model, N)
        assert tuple(out.shape) == (3, N, 1) and out.dtype == torch.float32
        assert calls == expect, calls

    run(expect=old)                                    # default: off
    model.set_fused_tail(True)
    run(expect=new)                                    # four calls per block, ln_1 once, the head last
    run(grad=True, expect=old)                         # an autograd graph is being recorded
    if which != 2:                                     # the 3-D model refuses bf16 storage altogether
        model.set_engine("bf16s")
        run(expect=old)
        model.set_engine("split")
    monkeypatch.setattr(ops, "block_tail_supported", lambda *a, **k: False)
    run(expect=old)
    monkeypatch.undo()
    calls = _record(monkeypatch)
    for b in model.blocks:                             # a generic MLP (hidden layers) keeps the default route
        b.mlp.linears.append(torch.nn.Sequential(torch.nn.Linear(b.mlp.n_hidden, b.mlp.n_hidden), torch.nn.GELU()))
    del calls[:]
    with torch.no_grad():
        _forward(model, N)
    assert "block_tail_fwd" not in calls and calls.count("deslice_fwd") == 2


def test_functional_block_tail_refuses_autograd():
    from transformerbasednavierstokesolver_amd import functional as Fn
    model, N = next(_models())
    b = model.blocks[0]
    fx = torch.zeros(1, N, 64, requires_grad=True)
    P = dict(zip(Fn.ATTN_KEYS, b.Attn.attention_parameters()))
    with pytest.raises(RuntimeError, match="no backward"):
        Fn.block_tail(fx, fx, P, 5, 7, 4, b.ln_2.weight, b.ln_2.bias, "gelu", b.mlp.linear_pre[0].weight,
                      b.mlp.linear_pre[0].bias, b.mlp.linear_post.weight, b.mlp.linear_post.bias)
