"""LearnSlice on the MI355X: the point-feature slice-weight stage and the loss stage element by element against a torch
float64 restatement (tests/learnslice_restatement.py), the module, SequenSolver.solve_with_slice_learner and the training
step against the reference's results in tests/golden/G11_learnslice.npz (written by tools/make_golden_learnslice.py).

Bounds.  The stage has no calibrated entry in elementwise_check.TAU / ROW_TOL, so the rule of test_gpu_sequensolver.py for
such stages applies: the yardstick is the same restatement evaluated by torch in float32 on the CPU against its float64
result on the test's own inputs, and the bound is 4 x its worst row error; every test prints the measured GPU value beside
the bound before it asserts.  The gradient of the last bias is exactly zero (it shifts the M logits of a point alike) and
is bounded absolutely by 8 eps32 sum p (|g| + |<p, g>|), as there.  Against G11 the yardstick is the reference's own float32
run, stored beside its float64 run.

Measured on one MI355X box (worst GPU row rel-L2 / its bound = 4 x the float32 CPU yardstick, at the case where the ratio is
largest; B N M C P):

  point_sw  sw     1.55e-06 / 5.88e-06   2 30 16 32 2        point_sw  dw3    6.66e-07 / 2.50e-06   2 30 16 32 2
  point_sw  dcode  6.62e-05 / 9.26e-05   3 30 16 32 3        point_sw  db3 (absolute)  5.22e-07 / 1.65e-05   1 30 128 64 128
  point_sw  dw1    4.09e-06 / 9.42e-06   2 30 16 32 2        slice_mse loss   2.66e-08 / 1.06e-07   B=2 N=30 M=16
  point_sw  db1    7.21e-07 / 2.62e-06   2 30 16 32 2        slice_mse dsw    1.01e-07 / 4.03e-07   B=1 N=4099 M=128
  point_sw  dw2    2.84e-06 / 7.25e-06   2 30 16 32 2        functional nodes (2 30 16 32 12): loss 6.68e-08 / 4.21e-07,
  point_sw  db2    5.71e-07 / 2.08e-06   2 30 16 32 2          worst gradient dw2 6.16e-07 / 3.66e-06

The small cases sit closest to their bounds because their yardstick is small (few rows, short sums): at N = 4096 / 4099 every
quantity uses under a third of its bound (worst: dcode 5.28e-06 / 1.68e-05 at 1 4096 16 32 64).  Against G11 (the bound is
4 x the reference's own float32 error), worst over the three checkpoints: slice weights 2.10e-07 / 8.53e-07 (P = 2),
training-step loss 5.66e-09 / 2.26e-08 (P = 74), worst gradient linear_pre.0.weight 1.98e-06 / 4.10e-06 (P = 64), |db3| at most
5.7e-09 against 1.4e-07.  solve_with_slice_learner: output 6.17e-07 (P = 2) and 8.78e-07 (P = 74) against 1e-05 on both
engines, learned weights 2.75e-07 / 9.70e-07 and 5.66e-07 / 3.48e-06.  Training step on the tiny model: losses within 3e-07
and the five parameters within 5.1e-08 of the float64 restatement (bound 2e-05) with either optimizer; the last bias moved by
at most 1.15e-03 (bound 2 lr = 2e-03).
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_l2
from elementwise_check import poisoned
import learnslice_restatement as L
import sequensolver_restatement as R
from test_gpu_sequensolver import EPS32, PNAMES, _bounded, _point_sw_operands, _sw_restated
from test_sequensolver_host import TINY_ENCODER

pytestmark = pytest.mark.gpu

UNSUP, ARG = 1002, 1001
G10 = os.path.join(GOLDEN, "G10_sequensolver.npz")
G11 = os.path.join(GOLDEN, "G11_learnslice.npz")
CHECKPOINTS = {"pos": (0, 0), "unified": (1, 0), "unified_vort": (1, 1)}      # unified_pos, use_vorticity
B3 = L.KEYS[5]


@pytest.fixture(scope="module")
def g10():
    return np.load(G10)


@pytest.fixture(scope="module")
def g11():
    return np.load(G11)


# ---------------------------------------------------------------------------------------------- the stage
POINT_SW_CASES = [      # B, N, M, C, P
    (1, 1, 8, 16, 1), (2, 30, 16, 32, 2), (3, 30, 16, 32, 3), (1, 257, 16, 32, 12), (2, 30, 5, 16, 64),
    (1, 4096, 16, 32, 64), (1, 4099, 16, 32, 74), (1, 257, 100, 32, 74), (1, 30, 128, 64, 128), (2, 4099, 8, 64, 128),
]


def _point_sw_restated(code, feat, params, dsw, dtype):
    return _sw_restated(L.point_slice_weights, code, feat, params, dsw, dtype)


@pytest.mark.parametrize("B,N,M,C,P", POINT_SW_CASES)
def test_point_slice_weights_forward_backward_rows(B, N, M, C, P):
    from transformerbasednavierstokesolver_amd import ops
    code, feat, params, dsw = _point_sw_operands(B, N, M, C, P, seed=3000 + N + 3 * M + C + B + 5 * P)
    sw64, dcode64, g64, dl_sum = _point_sw_restated(code, feat, params, dsw, torch.float64)
    sw32, dcode32, g32, _ = _point_sw_restated(code, feat, params, dsw, torch.float32)
    dev = [t.cuda() for t in (code, feat, dsw)]
    Pd = tuple(p.cuda() for p in params)
    label = f"point_sw B={B} N={N} M={M} C={C} P={P}"
    sw = poisoned(ops.point_slice_weights_fwd, dev[0], dev[1], Pd)
    assert sw.shape == (B, 1, N, M)
    _bounded("sw", sw, sw64, sw32, label)
    assert float((sw.sum(-1) - 1).abs().max()) < 1e-5
    dcode, *grads = poisoned(ops.point_slice_weights_bwd, dev[0], dev[1], Pd, dev[2])
    _bounded("dcode", dcode, dcode64, dcode32, label)
    for name, got, r64, r32 in zip(PNAMES[:5], grads, g64, g32):
        _bounded(name, got, r64, r32, label)
    bound = 8 * EPS32 * dl_sum
    print(f"{label} db3: GPU |db3| {float(grads[5].abs()):.3g}, bound {bound:.3g} (true value 0)")
    assert float(grads[5].abs()) <= bound
    # accumulate: adding into zeros gives the same bits, adding into the result doubles it exactly; no dcode on request
    zeros = tuple(torch.zeros_like(g) for g in grads)
    none, *acc0 = ops.point_slice_weights_bwd(dev[0], dev[1], Pd, dev[2], need_dcode=False, into=zeros)
    assert none is None and all(torch.equal(a, g) for a, g in zip(acc0, grads))
    twice = tuple(g.clone() for g in grads)
    ops.point_slice_weights_bwd(dev[0], dev[1], Pd, dev[2], into=twice)
    assert all(torch.equal(t, 2 * g) for t, g in zip(twice, grads))
    # a second run gives the same bits
    assert torch.equal(ops.point_slice_weights_fwd(dev[0], dev[1], Pd), sw)
    dcode2, *grads2 = ops.point_slice_weights_bwd(dev[0], dev[1], Pd, dev[2])
    assert torch.equal(dcode2, dcode) and all(torch.equal(a, g) for a, g in zip(grads2, grads))


# ---------------------------------------------------------------------------------------------- the loss
@pytest.mark.parametrize("B,N,M", [(1, 1, 5), (2, 30, 16), (1, 4099, 128)])
def test_slice_mse_value_and_gradient(B, N, M):
    from transformerbasednavierstokesolver_amd import ops
    g = torch.Generator().manual_seed(4000 + N + M + B)
    sw = torch.softmax(2 * torch.randn(B, 1, N, M, generator=g), -1)
    target = torch.softmax(2 * torch.randn(B, 1, N, M, generator=g), -1)
    gout = torch.randn(1, generator=g)

    def restated(dtype):
        s = sw.to(dtype).clone().requires_grad_(True)
        loss = L.slice_mse(s, target.to(dtype))
        loss.backward(gout.to(dtype).reshape(()))
        return loss.detach().reshape(1), s.grad

    l64, d64 = restated(torch.float64)
    l32, d32 = restated(torch.float32)
    label = f"slice_mse B={B} N={N} M={M}"
    loss = poisoned(ops.slice_mse_fwd, sw.cuda(), target.cuda())
    assert loss.shape == (1,)
    _bounded("loss", loss, l64, l32, label)
    dsw = poisoned(ops.slice_mse_bwd, sw.cuda(), target.cuda(), gout.cuda())
    _bounded("dsw", dsw, d64, d32, label)
    assert torch.equal(ops.slice_mse_fwd(sw.cuda(), target.cuda()), loss)
    assert torch.equal(ops.slice_mse_bwd(sw.cuda(), target.cuda(), gout.cuda()), dsw)


def test_functional_nodes_backpropagate():
    """functional.point_slice_weights and slice_mse as autograd nodes: the gradients of the composed loss against float64."""
    from transformerbasednavierstokesolver_amd import functional as Fn
    code, feat, params, _ = _point_sw_operands(2, 30, 16, 32, 12, seed=77)
    target = torch.softmax(torch.randn(2, 1, 30, 16, generator=torch.Generator().manual_seed(78)), -1)

    def restated(dtype):
        c = code.to(dtype).clone().requires_grad_(True)
        P = [p.to(dtype).clone().requires_grad_(True) for p in params]
        loss = L.slice_mse(L.point_slice_weights(c, feat.to(dtype), *P), target.to(dtype))
        loss.backward()
        return [loss.detach().reshape(1), c.grad] + [p.grad for p in P]

    r64, r32 = restated(torch.float64), restated(torch.float32)
    c = code.cuda().requires_grad_(True)
    P = [p.cuda().requires_grad_(True) for p in params]
    f = feat.cuda().requires_grad_(True)
    loss = Fn.slice_mse(Fn.point_slice_weights(c, f, *P), target.cuda())
    assert loss.dim() == 0
    loss.backward()
    assert f.grad is None                                                   # the features get no gradient
    got = [loss.detach().reshape(1), c.grad] + [p.grad for p in P]
    for name, a, b64, b32 in zip(("loss", "dcode") + PNAMES[:5], got, r64, r32):
        _bounded(name, a, b64, b32, "functional B=2 N=30 M=16 C=32 P=12")


# ---------------------------------------------------------------------------------------------- refusals and B = 0
def test_point_slice_weights_refusals_and_empty_batch():
    from transformerbasednavierstokesolver_amd import _lib, ops
    lib = _lib.load()
    f = lib.pa2d_point_slice_weights_fwd
    nul = [0] * 9
    assert f(*nul, 1, 30, 16, 32, 0, 64, 1, 0, 0, 0) == UNSUP           # P = 0
    assert f(*nul, 1, 30, 16, 32, 129, 64, 1, 0, 0, 0) == UNSUP         # P = 129
    assert f(*nul, 1, 30, 16, 12, 74, 64, 1, 0, 0, 0) == UNSUP          # C = 12
    assert f(*nul, 1, 30, 129, 32, 74, 64, 1, 0, 0, 0) == UNSUP         # M = 129
    assert f(*nul, 1, 30, 16, 32, 74, 128, 1, 0, 0, 0) == UNSUP         # hidden width 128
    assert f(*nul, 1, 30, 16, 32, 74, 64, 2, 0, 0, 0) == UNSUP          # two hidden layers
    assert f(*nul, 1, 0, 16, 32, 74, 64, 1, 0, 0, 0) == ARG             # N = 0
    assert f(*nul, 0, 30, 16, 32, 74, 64, 1, 0, 0, 0) == 0              # B = 0
    code, feat, params, _ = _point_sw_operands(1, 30, 16, 32, 74, seed=5)
    P = tuple(p.cuda() for p in params)
    wide = (torch.randn(128, 106), torch.randn(128), torch.randn(128, 128), torch.randn(128), torch.randn(1, 128), params[5])
    with pytest.raises(RuntimeError, match="PA2D_ERR_UNSUPPORTED"):
        ops.point_slice_weights_fwd(code.cuda(), feat.cuda(), tuple(p.cuda() for p in wide))
    big = (torch.randn(64, 32 + 129),) + params[1:]
    with pytest.raises(RuntimeError, match="PA2D_ERR_UNSUPPORTED"):
        ops.point_slice_weights_fwd(code.cuda(), torch.rand(1, 30, 129).cuda(), tuple(p.cuda() for p in big))
    with pytest.raises(ValueError, match="C\\+P"):
        ops.point_slice_weights_fwd(code.cuda(), torch.rand(1, 30, 64).cuda(), P)
    with pytest.raises(ValueError, match="dsw must be"):
        ops.point_slice_weights_bwd(code.cuda(), feat.cuda(), P, torch.zeros(1, 1, 30, 8).cuda())
    # B = 0: parameter gradients are exact zeros (overwrite) or untouched (accumulate)
    e_code, e_feat, e_dsw = (torch.empty(0, 16, 32).cuda(), torch.empty(0, 30, 74).cuda(), torch.empty(0, 1, 30, 16).cuda())
    assert ops.point_slice_weights_fwd(e_code, e_feat, P).shape == (0, 1, 30, 16)
    dcode, *g = poisoned(ops.point_slice_weights_bwd, e_code, e_feat, P, e_dsw)
    assert dcode.shape == (0, 16, 32) and all(float(t.abs().sum()) == 0.0 for t in g)
    ones = tuple(torch.ones_like(t) for t in g)
    ops.point_slice_weights_bwd(e_code, e_feat, P, e_dsw, into=ones)
    assert all(bool((t == 1).all()) for t in ones)
    empty = torch.empty(0, 1, 30, 16).cuda()
    assert float(ops.slice_mse_fwd(empty, empty)) == 0.0 and ops.slice_mse_bwd(empty, empty, torch.ones(1).cuda()).shape == empty.shape


# ---------------------------------------------------------------------------------------------- the module against G11
def _learner(g11, name, **kw):
    from transformerbasednavierstokesolver_amd.LearnSlice import LearnSlice
    up, uv = CHECKPOINTS[name]
    m = LearnSlice(unified_pos=up, use_vorticity=uv, **kw)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in L.golden_checkpoint(g11, name).items()}, strict=True)
    return m.cuda()


def _fixture_rows(g11, key, got):
    """The stored every-7th-point rows of [1, 1, N, M] weights under 4 x the worst row error of the reference's float32 run."""
    stride = int(g11["points.stride"])
    ref64, ref32 = torch.from_numpy(g11[key + ".f64"]), torch.from_numpy(g11[key + ".f32"])
    _bounded(key, got[0, 0, ::stride], ref64, ref32, "G11")
    nrm = float(g11[key + ".norm.f64"])
    assert abs(float(got.double().norm()) - nrm) <= 1e-5 * nrm


@pytest.mark.parametrize("name", list(CHECKPOINTS))
def test_module_matches_reference(g11, name):
    m = _learner(g11, name)
    code, pos, fx, uv = L.golden_case_inputs(g11, name)
    code, pos, fx = (torch.from_numpy(a).cuda() for a in (code, pos, fx))
    with torch.no_grad():
        sw = m.get_slice_weight(code, pos, fx, use_vorticity=uv)
    assert sw.shape == (1, 1, 4096, 16)
    _fixture_rows(g11, f"case.{name}.sw", sw)
    # every sample of a batch uses its own code and features: B = 2 is the two B = 1 calls, bit for bit
    code2 = torch.cat((code, code.flip(2) * 0.5))
    pos2, fx2 = torch.cat((pos, pos.flip(1))), torch.cat((fx, -fx))
    with torch.no_grad():
        both = m.get_slice_weight(code2, pos2, fx2, use_vorticity=uv)
        second = m.get_slice_weight(code2[1:], pos2[1:], fx2[1:], use_vorticity=uv)
    assert torch.equal(both[0], sw[0]) and torch.equal(both[1], second[0]) and not torch.equal(both[1], both[0])
    # the reference's per-point call is row n of get_slice_weight
    feat = torch.cat((pos, fx), -1) if uv else pos
    with torch.no_grad():
        for n in (0, 1234, 4095):
            w = m(code[0, 0], feat[0, n:n + 1])
            assert w.shape == (1, 16) and torch.equal(w[0], sw[0, 0, n])
    # the 30-point training step: loss and the six gradients against the reference's float64 loop over the points
    idx, target = L.golden_train_target(g11, name)
    sd32 = {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in L.golden_checkpoint(g11, name).items()}
    loss32 = L.slice_mse(L.get_slice_weight(sd32, code.cpu(), pos.cpu()[:, idx], fx.cpu()[:, idx], uv), target.float())
    loss32.backward()
    from transformerbasednavierstokesolver_amd import functional as Fn
    loss = Fn.slice_mse(m.get_slice_weight(code, pos[:, idx].contiguous(), fx[:, idx].contiguous(), use_vorticity=uv),
                        target.float().cuda())
    loss.backward()
    want = torch.from_numpy(g11[f"case.{name}.train.loss"]).reshape(1)
    _bounded(f"case.{name}.train.loss", loss.detach().reshape(1), want, loss32.detach().reshape(1), "G11")
    grads = dict(m.named_parameters())
    for k in L.KEYS[:5]:
        _bounded(f"case.{name}.train.grad.{k}", grads[k].grad, torch.from_numpy(g11[f"case.{name}.train.grad.{k}"]),
                 sd32[k].grad, "G11")
    s, g = (t.double().cpu() for t in (m.get_slice_weight(code, pos[:, idx].contiguous(), fx[:, idx].contiguous(),
                                                          use_vorticity=uv).detach(), target))
    dsw = 2.0 / 16 * (s - g)
    bound = 8 * EPS32 * float((s * (dsw.abs() + (s * dsw).sum(-1, keepdim=True).abs())).sum())
    print(f"G11 case.{name}.train db3: GPU {float(grads[L.KEYS[5]].grad.abs()):.3g}, bound {bound:.3g} (true value 0)")
    assert float(grads[L.KEYS[5]].grad.abs()) <= bound


# ---------------------------------------------------------------------------------------------- solve_with_slice_learner
def _solve_setup(g10, g11, case, engine):
    from test_gpu_sequensolver import _golden_model
    cfg = json.loads(str(g11[f"solve.{case}.config"]))
    name = cfg["checkpoint"]
    m, (pos, fx, y, _) = _golden_model(g10, cfg["g10_case"], engine)
    pos, fx, y = pos[:1].contiguous(), fx[:1].contiguous(), y[:1].contiguous()
    up, uv = CHECKPOINTS[name]
    if up:
        pos = torch.from_numpy(L.unified_distances()).cuda()
    return m, name, pos, fx, y, up, uv


@pytest.mark.parametrize("engine", [None, "f32"])
@pytest.mark.parametrize("case", ["pos", "vort"])
def test_solve_with_slice_learner_matches_reference(g10, g11, case, engine):
    m, name, pos, fx, y, up, uv = _solve_setup(g10, g11, case, engine)
    sd = {k: torch.from_numpy(v) for k, v in L.golden_checkpoint(g11, name).items()}
    label = f"G11 solve {case} engine={engine}"
    with torch.no_grad():
        out = m.solve_with_slice_learner(sd, pos, fx, y, unified_pos=up, use_vorticity=uv)
    assert out.shape == (1, 4096, 1)
    base, own = 1e-5, float(g11[f"solve.{case}.fp32_self_error.out"])      # the rule of the G10 model tests
    bound = 4 * own if own > base / 4 else base
    err = L.rel(out, g11[f"solve.{case}.out.f64"])
    print(f"{label} out: rel-L2 {err:.3g}, bound {bound:.3g}")
    assert err <= bound
    _fixture_rows(g11, f"solve.{case}.learned", m.learned_slice_weights)
    assert torch.equal(m.slice_weights, m.encoder.get_attention_slice())          # decoded with the true frame's weights
    assert not torch.equal(m.slice_weights, m.learned_slice_weights)
    # a LearnSlice instance and a checkpoint file give the same bits as the state_dict
    learner = _learner(g11, name).train()
    with torch.no_grad():
        assert torch.equal(m.solve_with_slice_learner(learner, pos, fx, y, use_vorticity=uv), out)
        assert learner.training and all(p.requires_grad for p in learner.parameters())      # the caller's module is left alone
        # decode_with_learned: decode() of the same code with the learned weights
        out_l = m.solve_with_slice_learner(learner, pos, fx, y, use_vorticity=uv, decode_with_learned=True)
        assert torch.equal(m.slice_weights, m.learned_slice_weights)
        from transformerbasednavierstokesolver_amd import functional as Fn
        want = Fn.head(Fn.layer_norm(m.decode(m.code), m.ln_3.weight, m.ln_3.bias), m.mlp2.weight, m.mlp2.bias)
    assert torch.equal(out_l, want) and not torch.equal(out_l, out)
    for mode in (dict(use_previous_slice=True), dict(learn_from_vort=True)):
        with pytest.raises(NotImplementedError, match="forward_previous_slice"):
            m.solve_with_slice_learner(sd, pos, fx, y, unified_pos=up, use_vorticity=uv, **mode)


def test_solve_with_slice_learner_from_a_file_and_a_batch(g10, g11, tmp_path):
    m, name, pos, fx, y, up, uv = _solve_setup(g10, g11, "pos", None)
    sd = {k: torch.from_numpy(v) for k, v in L.golden_checkpoint(g11, name).items()}
    path = tmp_path / "slice.pt"
    torch.save(sd, path)
    with torch.no_grad():
        one = m.solve_with_slice_learner(sd, pos, fx, y)
        assert torch.equal(m.solve_with_slice_learner(str(path), pos, fx, y), one)
        # any B: sample 0 of a batch of two is the B = 1 call up to the batched GEMMs' tiling
        two = m.solve_with_slice_learner(sd, pos.repeat(2, 1, 1), torch.cat((fx, fx.flip(1))), torch.cat((y, y.flip(1))))
    assert two.shape == (2, 4096, 1) and m.learned_slice_weights.shape == (2, 1, 4096, 16)
    assert rel_l2(two[:1], one) <= 1e-5


# ---------------------------------------------------------------------------------------------- the training step
def _restated_training(sd_seq, sd_ls, x, fx, yy, use_vorticity, hyper, dtype):
    """LearnSlice.py:477-526 on the tiny model in `dtype` with torch.optim.AdamW: (losses, final parameters)."""
    seq = {k: v.to(dtype) for k, v in sd_seq.items()}
    enc, own = R.split_state_dict(seq)
    params = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd_ls.items()}
    opt = torch.optim.AdamW([params[k] for k in L.KEYS], lr=hyper["lr"], weight_decay=hyper["weight_decay"])
    x, fx, yy = x.to(dtype), fx.to(dtype), yy.to(dtype)
    B, N, T = fx.shape
    losses = []
    for t in range(yy.shape[-1]):
        y = yy[..., t:t + 1]
        with torch.no_grad():
            target = R.encode(enc, TINY_ENCODER, x, y)[1]
            codes = [R.encode(enc, TINY_ENCODER, x, fx[:, :, i:i + 1])[0] for i in range(T)]
            tokens = torch.stack([c.reshape(B, -1) for c in codes], 1)
            code = R.tokens_to_code(own, tokens, 2, tokens.shape[-1] ** -0.5).reshape(B, 1, 8, 16)
        loss = L.slice_mse(L.get_slice_weight(params, code, x, fx, use_vorticity), target)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        fx = torch.cat((fx[..., 1:], y), dim=-1)
    return losses, {k: v.detach() for k, v in params.items()}


@pytest.mark.parametrize("use_vorticity", [0, 1])
def test_learnslice_train_step_on_a_tiny_model(use_vorticity):
    """6 x 5 mesh, M = 8, C = 16, T = 2, two output frames, B = 3: losses and parameters after the two steps against the
    float64 restatement with torch.optim.AdamW to 2e-5 (the figure of the SequenSolver training test), with torch's AdamW
    and with FusedAdamW; the frozen SequenSolver is left unchanged.

    The last bias is the exception.  It shifts the M logits of a point alike, so the slice weights do not depend on it and
    its true gradient is 0: the float64 restatement sees 1e-18 and leaves it where it was, any float32 evaluation (the
    reference's own included) sees rounding noise of 1e-8, and Adam's g / (|g| + eps) turns noise of the size of its eps
    into a step of up to lr.  Its value after two steps is therefore bounded by those two steps, 2 lr, not by 2e-5; nothing
    else depends on it, and the losses (which are checked) show that."""
    from transformerbasednavierstokesolver_amd import harness
    from transformerbasednavierstokesolver_amd.LearnSlice import LearnSlice
    from transformerbasednavierstokesolver_amd.SequenSolver import SequenSolver
    from transformerbasednavierstokesolver_amd.optim import FusedAdamW
    hyper = dict(lr=1e-3, weight_decay=1e-5)
    torch.manual_seed(11)
    seq = SequenSolver(None, T=2, W=5, H=6, M=8, C=16, B=3, layers=2, encoder_config=TINY_ENCODER)
    ls = LearnSlice(0, use_vorticity, C=16, M=8, T=2)
    with torch.no_grad():
        ls.weight_projection.linear_post.weight.mul_(4.0)
    sd_seq = {k: v.detach().clone() for k, v in seq.state_dict().items()}
    sd_ls = {k: v.detach().clone() for k, v in ls.state_dict().items()}
    g = torch.Generator().manual_seed(12)
    x, fx, yy = torch.rand(3, 30, 2, generator=g), torch.randn(3, 30, 2, generator=g), torch.randn(3, 30, 2, generator=g)
    want_losses, want = _restated_training(sd_seq, sd_ls, x, fx, yy, use_vorticity, hyper, torch.float64)
    seq = seq.cuda().eval()
    for p in seq.parameters():
        p.requires_grad = False
    results = {}
    for kind in ("torch", "fused"):
        m = LearnSlice(0, use_vorticity, C=16, M=8, T=2)
        m.load_state_dict(sd_ls, strict=True)
        m = m.cuda().train()
        if kind == "torch":
            opt, sync = torch.optim.AdamW(m.parameters(), **hyper), None
        else:
            opt = FusedAdamW(m.parameters(), **hyper)
            sync = opt.sync
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda step: 1.0)
        losses = harness.learnslice_train_step(m, opt, sched, seq, x.cuda(), fx.cuda(), yy.cuda(), use_vorticity, grad_sync=sync)
        assert len(losses) == 2 and sched.last_epoch == 2                 # one optimizer step per frame
        losses = [float(v) for v in losses]
        print(f"learnslice_train_step use_vorticity={use_vorticity} {kind}: losses {losses} against {want_losses}")
        np.testing.assert_allclose(losses, want_losses, rtol=2e-5)
        got = {k: v.detach().clone() for k, v in m.state_dict().items()}
        for k in L.KEYS[:5]:
            err = rel_l2(got[k], want[k])
            print(f"  {kind} {k}: rel-L2 {err:.3g}")
            assert err <= 2e-5, (kind, k, err)
            assert not torch.equal(got[k].cpu(), sd_ls[k]), k              # every parameter moved
        # this bounds the last bias by what Adam can do in two steps and nothing more: Adam normalises whatever gradient it
        # is given.  What holds its gradient near its true value 0 is the absolute db3 bound of the stage tests above.
        moved = float((got[B3].cpu().double() - want[B3]).abs().max())
        print(f"  {kind} {B3}: |difference| {moved:.3g}, bound {2 * hyper['lr']:.3g} (see the docstring)")
        assert moved <= 2 * hyper["lr"]
        results[kind] = (losses, got)
    np.testing.assert_allclose(results["fused"][0], results["torch"][0], rtol=2e-5)
    for k in L.KEYS[:5]:
        assert rel_l2(results["fused"][1][k], results["torch"][1][k]) <= 2e-5, k
    for k, v in seq.state_dict().items():
        assert torch.equal(v.cpu(), sd_seq[k]), k
