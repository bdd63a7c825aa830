"""LearnSlice without a GPU: the new C ABI symbols with their host-side refusals, the shape errors of the ops, the module's
interface against the reference (tests/golden/G11_learnslice.npz, written by tools/make_golden_learnslice.py), and the fixture's
float64 results against the torch float64 restatement of tests/learnslice_restatement.py (an oracle-vs-golden check, like
test_sequensolver_host.py: both sides are float64, so they meet to 1e-12)."""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import learnslice_restatement as L

G11 = os.path.join(GOLDEN, "G11_learnslice.npz")
NEW_SYMBOLS = {      # name: number of arguments in include/pa2d.h
    "pa2d_point_slice_weights_fwd": 19,
    "pa2d_point_slice_weights_bwd_workspace": 5,
    "pa2d_point_slice_weights_bwd": 29,
    "pa2d_slice_mse_workspace": 2,
    "pa2d_slice_mse_fwd": 8,
    "pa2d_slice_mse_bwd": 7,
}
CHECKPOINTS = {"pos": (0, 0, 2), "unified": (1, 0, 64), "unified_vort": (1, 1, 74)}      # unified_pos, use_vorticity, P
ARG, UNSUP, WS = 1001, 1002, 1003


@pytest.fixture(scope="module")
def g11():
    return np.load(G11)


def test_c_abi_symbols_bound_with_header_arity():
    from transformerbasednavierstokesolver_amd import _lib
    _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "pa2d.h")).read()
    flat = " ".join(header.split())
    for name, arity in NEW_SYMBOLS.items():
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == arity, name
        decl = flat.split(name + "(", 1)[1].split(")", 1)[0]
        assert len(decl.split(",")) == arity, name
        assert "LearnSlice.py:" in header.split(name + "(", 1)[0].rsplit("/* ----", 1)[1], name     # cites its lines


def test_host_side_refusals_with_null_pointers():
    from transformerbasednavierstokesolver_amd import _lib
    lib = _lib.load()
    # pa2d_point_slice_weights_fwd(code, feat, w1, b1, w2, b2, w3, b3, sw, B, N, M, C, P, hidden, depth, stream, ev0, ev1)
    f = lib.pa2d_point_slice_weights_fwd
    nul = [0] * 9
    assert f(*nul, 1, 4096, 16, 32, 0, 64, 1, 0, 0, 0) == UNSUP         # P = 0
    assert f(*nul, 1, 4096, 16, 32, 129, 64, 1, 0, 0, 0) == UNSUP       # P = 129
    assert f(*nul, 1, 4096, 16, 12, 74, 64, 1, 0, 0, 0) == UNSUP        # C = 12
    assert f(*nul, 1, 4096, 129, 32, 74, 64, 1, 0, 0, 0) == UNSUP       # M = 129
    assert f(*nul, 1, 4096, 0, 32, 74, 64, 1, 0, 0, 0) == UNSUP         # M = 0
    assert f(*nul, 1, 4096, 16, 32, 74, 128, 1, 0, 0, 0) == UNSUP       # hidden width 128
    assert f(*nul, 1, 4096, 16, 32, 74, 64, 2, 0, 0, 0) == UNSUP        # two hidden layers
    assert f(*nul, 1, 0, 16, 32, 74, 64, 1, 0, 0, 0) == ARG             # N = 0
    assert f(*nul, -1, 4096, 16, 32, 74, 64, 1, 0, 0, 0) == ARG
    assert f(*nul, 1, 4096, 16, 32, 74, 64, 1, 0, 0, 0) == ARG          # supported shape, null pointers
    assert f(*nul, 0, 4096, 16, 32, 74, 64, 1, 0, 0, 0) == 0            # B = 0: no-op
    assert f(*nul, 1 << 16, 1 << 16, 16, 32, 74, 64, 1, 0, 0, 0) == UNSUP      # > 4 GiB of features
    for P in (1, 2, 3, 12, 64, 74, 128):
        assert f(*nul, 0, 30, 128, 64, P, 64, 1, 0, 0, 0) == 0
    # pa2d_point_slice_weights_bwd(8 inputs, dsw, dcode, 6 gradients, ws, ws_bytes, B, N, M, C, P, hidden, depth,
    #                              accumulate, stream, ev0, ev1)
    b = lib.pa2d_point_slice_weights_bwd
    assert b(*([0] * 18), 1, 4096, 16, 32, 0, 64, 1, 0, 0, 0, 0) == UNSUP
    assert b(*([0] * 18), 1, 4096, 16, 32, 129, 64, 1, 0, 0, 0, 0) == UNSUP
    assert b(*([0] * 18), 1, 4096, 16, 12, 74, 64, 1, 0, 0, 0, 0) == UNSUP
    assert b(*([0] * 18), 1, 4096, 129, 32, 74, 64, 1, 0, 0, 0, 0) == UNSUP
    assert b(*([0] * 18), 1, 4096, 16, 32, 74, 128, 1, 0, 0, 0, 0) == UNSUP
    assert b(*([0] * 18), 1, 4096, 16, 32, 74, 64, 2, 0, 0, 0, 0) == UNSUP
    assert b(*([0] * 18), 1, 0, 16, 32, 74, 64, 1, 0, 0, 0, 0) == ARG
    assert b(*([16] * 16), 0, 0, 1, 4096, 16, 32, 74, 64, 1, 0, 0, 0, 0) == WS
    assert b(*([0] * 18), 0, 4096, 16, 32, 74, 64, 1, 1, 0, 0, 0) == 0                  # B = 0, accumulate: untouched
    ws = lib.pa2d_point_slice_weights_bwd_workspace
    assert ws(1, 4096, 16, 32, 74) > 0 and ws(0, 4096, 16, 32, 74) == 0
    assert ws(1, 4096, 129, 32, 74) == 0 and ws(1, 4096, 16, 32, 129) == 0
    assert ws(3, 4099, 128, 64, 128) >= 3 * 4099 * 64 * 4                               # holds dpf [B, N, 64]
    # pa2d_slice_mse_fwd(sw, target, loss, ws, ws_bytes, rows, M, stream) / _bwd(sw, target, gout, dsw, rows, M, stream)
    assert lib.pa2d_slice_mse_fwd(0, 0, 0, 0, 0, 30, 0, 0) == ARG
    assert lib.pa2d_slice_mse_fwd(0, 0, 0, 0, 0, -1, 16, 0) == ARG
    assert lib.pa2d_slice_mse_fwd(0, 0, 0, 0, 0, 30, 16, 0) == ARG
    assert lib.pa2d_slice_mse_fwd(16, 16, 16, 0, 0, 30, 16, 0) == WS
    assert lib.pa2d_slice_mse_bwd(0, 0, 0, 0, 30, 16, 0) == ARG
    assert lib.pa2d_slice_mse_bwd(0, 0, 0, 0, 0, 16, 0) == 0
    assert lib.pa2d_slice_mse_workspace(30, 16) > 0 and lib.pa2d_slice_mse_workspace(0, 16) == 0


def test_ops_shape_errors_and_cpu_tensors():
    from transformerbasednavierstokesolver_amd import ops
    P6 = lambda width: (torch.zeros(64, width), torch.zeros(64), torch.zeros(64, 64), torch.zeros(64), torch.zeros(1, 64),
                        torch.zeros(1))
    code, feat = torch.zeros(1, 8, 16), torch.zeros(1, 5, 74)
    good = P6(16 + 74)
    with pytest.raises(ValueError, match="C\\+P"):
        ops.point_slice_weights_fwd(code, feat, P6(16 + 2))                 # w1 is C+2 wide, the features 74
    with pytest.raises(ValueError, match="C\\+P"):
        ops.point_slice_weights_fwd(code, feat, good[:2] + (torch.zeros(64, 32),) + good[3:])
    with pytest.raises(ValueError, match="\\[B, N, P\\]"):
        ops.point_slice_weights_fwd(code, torch.zeros(5, 74), good)
    with pytest.raises(ValueError, match="\\[B, N, P\\]"):
        ops.point_slice_weights_fwd(code, torch.zeros(2, 5, 74), good)      # batch sizes differ
    with pytest.raises(ValueError, match="C\\+P"):
        ops.point_slice_weights_bwd(code, feat, P6(16 + 2), torch.zeros(1, 1, 5, 8))
    with pytest.raises(ValueError, match="dsw must be"):
        ops.point_slice_weights_bwd(code, feat, good, torch.zeros(1, 5, 8))
    with pytest.raises(ValueError, match="share a shape"):
        ops.slice_mse_fwd(torch.zeros(1, 1, 5, 8), torch.zeros(1, 1, 5, 4))
    with pytest.raises(ValueError, match="one value"):
        ops.slice_mse_bwd(torch.zeros(1, 1, 5, 8), torch.zeros(1, 1, 5, 8), torch.zeros(2))
    # well-shaped operands on the CPU: there is no CPU path
    with pytest.raises(RuntimeError, match="GPU"):
        ops.point_slice_weights_fwd(code, feat, good)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.slice_mse_fwd(torch.zeros(1, 1, 5, 8), torch.zeros(1, 1, 5, 8))


# ---------------------------------------------------------------------------------------------- the module
def test_signatures_match_the_reference_prefix(g11):
    from transformerbasednavierstokesolver_amd.LearnSlice import LearnSlice
    for fn, key in ((LearnSlice.__init__, "signature.init"), (LearnSlice.get_slice_weight, "signature.get_slice_weight")):
        ref = [tuple(p) for p in json.loads(str(g11[key]))]
        params = [(k, p) for k, p in inspect.signature(fn).parameters.items() if k != "self"]
        ours = [(k, None if p.default is inspect.Parameter.empty else p.default) for k, p in params]
        assert ours[:len(ref)] == ref, key
        assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for _, p in params[len(ref):]), key
    extra = list(inspect.signature(LearnSlice.__init__).parameters.items())[4:]
    assert [(k, p.default) for k, p in extra] == [("C", 32), ("M", 16), ("T", 10)]


def test_point_width_state_dict_and_strict_load(g11):
    from transformerbasednavierstokesolver_amd.LearnSlice import LearnSlice
    widths = {(0, 0): 2, (0, 1): 12, (1, 0): 64, (1, 1): 74}
    for (up, uv), P in widths.items():
        m = LearnSlice(unified_pos=up, use_vorticity=uv)
        assert m.pos == P and m.weight_projection.linear_pre[0].in_features == 32 + P
        assert sorted(m.state_dict()) == sorted(L.KEYS) and len(m.state_dict()) == 6
    assert LearnSlice(0, 1, C=16, M=8, T=2).pos == 4
    for name, (up, uv, P) in CHECKPOINTS.items():
        sd = {k: torch.from_numpy(v) for k, v in L.golden_checkpoint(g11, name).items()}
        assert sd[L.KEYS[0]].shape == (64, 32 + P)
        m = LearnSlice(unified_pos=up, use_vorticity=uv)
        res = m.load_state_dict(sd, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        assert all(torch.equal(m.state_dict()[k], v) for k, v in sd.items())


def test_unbuilt_methods_raise_and_widths_are_checked():
    from transformerbasednavierstokesolver_amd.LearnSlice import LearnSlice
    m = LearnSlice()
    t = torch.zeros(1, 1, 16, 32)
    for call, what in ((lambda: m.forward_all(torch.zeros(30, 16, 34)), "concatenated"),
                       (lambda: m.forward_previous_slice(torch.zeros(1, 1, 30, 16), t), "weight_projection_form_slice"),
                       (lambda: m.forward_from_vorticity(torch.zeros(1, 30, 64), torch.zeros(1, 30, 10)), "in_project_x"),
                       (lambda: m.forward_from_vorticity_seperate(torch.zeros(1, 30, 64), torch.zeros(1, 30, 10), t),
                        "in_project_x_seperate")):
        with pytest.raises(NotImplementedError, match=what):
            call()
    with pytest.raises(ValueError, match="P = 2"):
        m.get_slice_weight(t, torch.zeros(1, 30, 64), None)
    with pytest.raises(ValueError, match="P = 2"):
        m.get_slice_weight(t, torch.zeros(1, 30, 2), torch.zeros(1, 30, 10), use_vorticity=1)


def test_solve_with_slice_learner_signature_and_unbuilt_modes():
    from transformerbasednavierstokesolver_amd.SequenSolver import SequenSolver
    params = list(inspect.signature(SequenSolver.solve_with_slice_learner).parameters.items())[1:]
    assert [(k, p.default) for k, p in params[:9]] == [
        ("slice_learner_path", inspect.Parameter.empty), ("spatial_pos", inspect.Parameter.empty),
        ("fx", inspect.Parameter.empty), ("y", inspect.Parameter.empty), ("unified_pos", 0), ("use_vorticity", 0),
        ("use_previous_slice", False), ("learn_from_vort", False), ("use_code_for_vorticity", False)]      # SequenSolver.py:182
    assert [(k, p.kind, p.default) for k, p in params[9:]] == [("decode_with_learned", inspect.Parameter.KEYWORD_ONLY, False)]
    from test_sequensolver_host import TINY_ENCODER
    m = SequenSolver(None, T=2, W=5, H=6, M=8, C=16, B=1, layers=2, encoder_config=TINY_ENCODER)
    assert m.learned_slice_weights is None
    x, fx, y = torch.zeros(1, 30, 2), torch.zeros(1, 30, 2), torch.zeros(1, 30, 1)
    for mode in (dict(use_previous_slice=True), dict(learn_from_vort=True)):
        with pytest.raises(NotImplementedError, match="forward_previous_slice"):
            m.solve_with_slice_learner({}, x, fx, y, **mode)
    with pytest.raises(RuntimeError, match="Missing key"):      # a state_dict without the six tensors is not a slice learner
        m.solve_with_slice_learner({}, x, fx, y)


# ---------------------------------------------------------------------------------------------- restatement vs golden
@pytest.mark.parametrize("name", list(CHECKPOINTS))
def test_float64_restatement_reproduces_the_fixture(g11, name):
    """Both sides float64: rel-L2 <= 1e-12 for the slice weights at the stored points, their norm, and the training step's
    loss and six gradients."""
    sd = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in L.golden_checkpoint(g11, name).items()}
    code, pos, fx, uv = (torch.from_numpy(a).double() if isinstance(a, np.ndarray) else a
                         for a in L.golden_case_inputs(g11, name))
    stride = int(g11["points.stride"])
    with torch.no_grad():
        sw = L.get_slice_weight(sd, code, pos, fx, uv)
    assert sw.shape == (1, 1, 4096, 16)
    assert L.rel(sw[0, 0, ::stride], g11[f"case.{name}.sw.f64"]) <= 1e-12
    assert abs(float(sw.norm()) - float(g11[f"case.{name}.sw.norm.f64"])) <= 1e-12 * float(sw.norm())
    # the float32 run of the reference is the yardstick of the GPU test: it must be a float32-sized distance away
    assert 1e-9 < L.rel(g11[f"case.{name}.sw.f32"], g11[f"case.{name}.sw.f64"]) < 1e-6
    idx, target = L.golden_train_target(g11, name)
    loss = L.slice_mse(L.get_slice_weight(sd, code, pos[:, idx], fx[:, idx], uv), target)
    loss.backward()
    assert abs(float(loss.detach()) - float(g11[f"case.{name}.train.loss"])) <= 1e-12 * float(loss.detach())
    for k in L.KEYS:
        if k == L.KEYS[5]:      # the last bias shifts every logit of a point alike: its true gradient is 0
            scale = float(sd[L.KEYS[4]].grad.norm())
            assert float(sd[k].grad.abs().max()) <= 1e-12 * scale and float(np.abs(g11[f"case.{name}.train.grad.{k}"]).max()) <= 1e-12 * scale
            continue
        assert L.rel(sd[k].grad, g11[f"case.{name}.train.grad.{k}"]) <= 1e-12, k


def test_fixture_holds_the_two_solve_cases(g11):
    for case, (ck, g10case) in (("pos", ("pos", "a")), ("vort", ("unified_vort", "b"))):
        cfg = json.loads(str(g11[f"solve.{case}.config"]))
        assert (cfg["checkpoint"], cfg["g10_case"], cfg["sample"]) == (ck, g10case, 0)
        assert g11[f"solve.{case}.out.f64"].shape == (4096,) and g11[f"solve.{case}.out.f64"].dtype == np.float64
        assert g11[f"solve.{case}.learned.f64"].shape == (586, 16)
        assert 0 < float(g11[f"solve.{case}.fp32_self_error.out"]) < 2.5e-6
    assert os.path.getsize(G11) <= 1_000_000
