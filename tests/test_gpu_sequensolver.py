"""SequenSolver on the MI355X: the two new stages element by element against a torch float64 restatement
(tests/sequensolver_restatement.py), and the whole model against the reference's results in
tests/golden/G10_sequensolver.npz (written by tools/make_golden_sequensolver.py).

Per-row bounds of the stages.  The two stages have no calibrated entry in elementwise_check.TAU / ROW_TOL.  Their
yardstick is the same restatement evaluated by torch in float32 on the CPU against its float64 result, on the test's
own inputs, and the bound is 4 x its worst row error (the margin the TAU table keeps over its measured values).  Every
test prints the measured GPU value beside the bound before it asserts.  The bias of the last layer of
weight_projection shifts all M logits of a point alike, so its true gradient is exactly zero and no relative bound
applies.  It is the sum over all rows of dlogit = p (g - <p, g>) (p the softmax, g the incoming gradient), whose terms
cancel within every point; each term is formed with a rounding error of about eps32 p (|g| + |<p, g>|), so the sum is
bounded by 8 eps32 sum p (|g| + |<p, g>|) (8: the handful of roundings per term).

Measured on one MI355X box (worst GPU row rel-L2 / its bound = 4 x the float32 CPU yardstick, at the case where the ratio is
largest; TAU-table style):

  seq_attn  out     1.02e-07 / 3.67e-07   B=5 T=10 dim=64           code_sw  sw     9.34e-07 / 1.20e-06   B=1 N=4096 M=128 C=16
  seq_attn  dq      5.39e-07 / 2.48e-06   B=5 T=32 dim=1024         code_sw  dcode  9.68e-05 / 1.03e-04   B=2 N=4096 M=32 C=64
  seq_attn  dk      3.13e-07 / 1.44e-06   B=1 T=32 dim=64           code_sw  dw1    1.21e-05 / 4.40e-05   B=1 N=257 M=100 C=32
  seq_attn  dv      1.18e-07 / 6.62e-07   B=5 T=3 dim=512           code_sw  db1    1.24e-06 / 2.78e-06   B=2 N=1 M=16 C=64
  seq_attn  out, no residual  1.85e-07 / 8.77e-07  B=5 T=10 dim=64  code_sw  dw2    9.89e-06 / 1.63e-05   B=3 N=30 M=5 C=16
  code_sw   db3 (absolute)    3.35e-08 / 1.34e-06  B=2 N=1 M=16     code_sw  db2    2.33e-06 / 4.55e-06   B=3 N=30 M=5 C=16
                                                                    code_sw  dw3    4.56e-06 / 8.82e-06   B=2 N=30 M=8 C=16

The code_sw cases run the point-feature kernels of test_gpu_learnslice.py with P = 2 (the two-coordinate entry points forward
to them) and are their coverage at N = 4096 / 4099; against the two-coordinate kernels the stage once had, only the two point
columns of dw1 changed bits, and no figure above moved.

The code gradient of the (2, 4096, 32, 64) case sits at 0.94 of its bound: that row is badly conditioned (rounding the
first-layer pre-activations or the hidden pre-activations z to float32 ONCE already moves it by 6e-6 and 1e-5), and the
kernel's fp32 sums of z are a few ulp worse than a blocked CPU GEMM's.  The model against G10 and the tiny model use at most
0.13 of their bounds (worst: the use_gt=False output of case a, 1.3e-06 against 1e-05; training losses 4e-8 against 2e-5)."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_l2
from elementwise_check import check_rows, poisoned
import sequensolver_restatement as R

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24
UNSUP, ARG, WS = 1002, 1001, 1003


def _rows(t):
    return t.reshape(1, -1) if t.dim() == 1 else t.reshape(-1, t.shape[-1])


def _row_err(a, b):
    """Worst row rel-L2 of a against b (both cast to float64)."""
    a, b = _rows(a.detach().double().cpu()), _rows(b.detach().double().cpu())
    return float(((a - b).norm(dim=1) / b.norm(dim=1).clamp_min(1e-300)).max())


def _bounded(name, got, ref64, ref32, label):
    """check_rows(got, ref64) under 4 x the worst row error of the float32 CPU restatement; prints both figures."""
    tol = 4.0 * _row_err(ref32, ref64)
    worst = _row_err(got, ref64)
    print(f"{label} {name}: GPU worst row rel-L2 {worst:.3g}, bound {tol:.3g}")
    check_rows(_rows(got), _rows(ref64), tol, label=f"{label} {name}")


# ---------------------------------------------------------------------------------------------- stage (a)
ATTN_CASES = [      # B, T, dim, factor on q (30: logits spread so wide that the softmax is near one-hot)
    (1, 1, 64, 1.0), (5, 3, 512, 1.0), (1, 10, 512, 1.0), (5, 32, 1024, 1.0), (1, 32, 64, 1.0), (5, 10, 1024, 1.0),
    (1, 3, 1024, 1.0), (5, 1, 512, 1.0), (1, 32, 512, 1.0), (5, 10, 64, 1.0), (2, 10, 512, 30.0),
]


def _attn_operands(B, T, dim, spread, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, T, dim, generator=g) * spread
    k, v, res, dout = (torch.randn(B, T, dim, generator=g) for _ in range(4))
    return q, k, v, res, dout


def _attn_restated(ops_in, dtype, scale):
    q, k, v, res = (t.to(dtype).clone().requires_grad_(True) for t in ops_in[:4])
    dout = ops_in[4].to(dtype)
    out = R.seq_attention(q, k, v, scale, res)
    out.backward(dout)
    return out.detach(), q.grad, k.grad, v.grad


@pytest.mark.parametrize("B,T,dim,spread", ATTN_CASES)
def test_sequence_attention_forward_backward_rows(B, T, dim, spread):
    from transformerbasednavierstokesolver_amd import ops
    cpu = _attn_operands(B, T, dim, spread, seed=1000 + 7 * T + dim + B)
    scale = dim ** -0.5
    ref64 = _attn_restated(cpu, torch.float64, scale)
    ref32 = _attn_restated(cpu, torch.float32, scale)
    q, k, v, res, dout = (t.cuda() for t in cpu)
    out, attn = poisoned(ops.seq_attn_fwd, q, k, v, scale, res)
    dq, dk, dv = poisoned(ops.seq_attn_bwd, q, k, v, attn, dout, scale)
    label = f"seq_attn B={B} T={T} dim={dim} spread={spread}"
    if spread > 1:
        assert float(attn.max(-1).values.median()) > 0.99, "the spread case is meant to be near one-hot"
    for name, got, r64, r32 in zip(("out", "dq", "dk", "dv"), (out, dq, dk, dv), ref64, ref32):
        _bounded(name, got, r64, r32, label)
    # without the residual the epilogue adds nothing: out - res of the restatement
    out0, _ = poisoned(ops.seq_attn_fwd, q, k, v, scale)
    no_res64 = R.seq_attention(*(t.double() for t in cpu[:3]), scale)
    no_res32 = R.seq_attention(*cpu[:3], scale)
    _bounded("out (no residual)", out0, no_res64, no_res32, label)


def test_sequence_attention_refusals_and_empty_batch():
    from transformerbasednavierstokesolver_amd import _lib, ops
    lib = _lib.load()
    # pa2d_seq_attn_fwd(q, k, v, res, out, attn, B, T, dim, scale, stream)
    assert lib.pa2d_seq_attn_fwd(0, 0, 0, 0, 0, 0, 1, 0, 64, 1.0, 0) == UNSUP          # T = 0
    assert lib.pa2d_seq_attn_fwd(0, 0, 0, 0, 0, 0, 1, 33, 64, 1.0, 0) == UNSUP         # T = 33
    assert lib.pa2d_seq_attn_fwd(0, 0, 0, 0, 0, 0, 1, 8, 66, 1.0, 0) == UNSUP          # dim % 4 != 0
    assert lib.pa2d_seq_attn_fwd(0, 0, 0, 0, 0, 0, 1, 8, 1028, 1.0, 0) == UNSUP        # beyond the LayerNorm limit
    assert lib.pa2d_seq_attn_bwd(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 33, 64, 1.0, 0) == UNSUP
    assert lib.pa2d_seq_attn_bwd(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 8, 30, 1.0, 0) == UNSUP
    assert lib.pa2d_seq_attn_fwd(0, 0, 0, 0, 0, 0, 0, 8, 64, 1.0, 0) == 0              # B = 0: no-op
    q = torch.randn(2, 33, 64, device="cuda")
    with pytest.raises(RuntimeError, match="PA2D_ERR_UNSUPPORTED"):
        ops.seq_attn_fwd(q, q, q, 1.0)
    e = torch.empty(0, 4, 64, device="cuda")
    out, attn = ops.seq_attn_fwd(e, e, e, 1.0)
    assert out.shape == (0, 4, 64) and attn.shape == (0, 4, 4)
    assert all(t.shape == (0, 4, 64) for t in ops.seq_attn_bwd(e, e, e, attn, e, 1.0))


# ---------------------------------------------------------------------------------------------- stage (b)
CODE_SW_CASES = [      # B, N, M, C
    (1, 1, 8, 16), (2, 30, 16, 32), (1, 4096, 16, 32), (1, 4099, 128, 64), (2, 4099, 8, 64), (1, 30, 32, 16),
    (2, 4096, 32, 64), (1, 30, 128, 32), (2, 1, 16, 64), (1, 4099, 32, 32), (2, 30, 8, 16), (1, 4096, 128, 16),
    (1, 257, 100, 32), (3, 30, 5, 16),          # slice counts that are no power of two
]
PNAMES = ("dw1", "db1", "dw2", "db2", "dw3", "db3")


def _point_sw_operands(B, N, M, C, P, seed):
    """Operands of the slice-weight stage with P features per point (test_gpu_learnslice.py draws its own from here)."""
    g = torch.Generator().manual_seed(seed)
    code = torch.randn(B, M, C, generator=g)
    feat = torch.rand(B, N, P, generator=g)
    params = (torch.randn(64, C + P, generator=g) * (2.0 / (C + P) ** 0.5), torch.randn(64, generator=g) * 0.1,
              torch.randn(64, 64, generator=g) * 0.2, torch.randn(64, generator=g) * 0.1,
              torch.randn(1, 64, generator=g) * 0.5, torch.randn(1, generator=g))
    dsw = torch.randn(B, 1, N, M, generator=g)
    return code, feat, params, dsw


def _code_sw_operands(B, N, M, C, seed):
    return _point_sw_operands(B, N, M, C, 2, seed)


def _sw_restated(restatement, code, feat, params, dsw, dtype):
    """`restatement` (R.code_slice_weights or learnslice_restatement.point_slice_weights) and its autograd in `dtype`."""
    code = code.to(dtype).clone().requires_grad_(True)
    P = [p.to(dtype).clone().requires_grad_(True) for p in params]
    sw = restatement(code, feat.to(dtype), *P)
    sw.backward(dsw.to(dtype))
    # sum p (|g| + |<p, g>|): the scale of the rounding in the (exactly zero) gradient of the last bias
    s, g = sw.detach(), dsw.to(dtype)
    scale = (s * (g.abs() + (s * g).sum(-1, keepdim=True).abs())).sum()
    return sw.detach(), code.grad, [p.grad for p in P], float(scale)


def _code_sw_restated(code, pos, params, dsw, dtype):
    return _sw_restated(R.code_slice_weights, code, pos, params, dsw, dtype)


@pytest.mark.parametrize("B,N,M,C", CODE_SW_CASES)
def test_code_slice_weights_forward_backward_rows(B, N, M, C):
    from transformerbasednavierstokesolver_amd import ops
    code, pos, params, dsw = _code_sw_operands(B, N, M, C, seed=2000 + N + 3 * M + C + B)
    sw64, dcode64, g64, dl_sum = _code_sw_restated(code, pos, params, dsw, torch.float64)
    sw32, dcode32, g32, _ = _code_sw_restated(code, pos, params, dsw, torch.float32)
    dev = [t.cuda() for t in (code, pos, dsw)]
    P = tuple(p.cuda() for p in params)
    label = f"code_sw B={B} N={N} M={M} C={C}"
    sw = poisoned(ops.code_slice_weights_fwd, dev[0], dev[1], P)
    assert sw.shape == (B, 1, N, M)
    _bounded("sw", sw, sw64, sw32, label)
    assert float((sw.sum(-1) - 1).abs().max()) < 1e-5
    dcode, *grads = poisoned(ops.code_slice_weights_bwd, dev[0], dev[1], P, dev[2])
    _bounded("dcode", dcode, dcode64, dcode32, label)
    for name, got, r64, r32 in zip(PNAMES[:5], grads, g64, g32):
        _bounded(name, got, r64, r32, label)
    bound = 8 * EPS32 * dl_sum
    print(f"{label} db3: GPU |db3| {float(grads[5].abs()):.3g}, bound {bound:.3g} (true value 0)")
    assert float(grads[5].abs()) <= bound
    # accumulate: adding into zeros gives the same bits, adding into the result doubles it exactly; no dcode on request
    zeros = tuple(torch.zeros_like(g) for g in grads)
    none, *acc0 = ops.code_slice_weights_bwd(dev[0], dev[1], P, dev[2], need_dcode=False, into=zeros)
    assert none is None and all(torch.equal(a, g) for a, g in zip(acc0, grads))
    twice = tuple(g.clone() for g in grads)
    ops.code_slice_weights_bwd(dev[0], dev[1], P, dev[2], into=twice)
    assert all(torch.equal(t, 2 * g) for t, g in zip(twice, grads))
    # a second run gives the same bits
    assert torch.equal(ops.code_slice_weights_fwd(dev[0], dev[1], P), sw)
    dcode2, *grads2 = ops.code_slice_weights_bwd(dev[0], dev[1], P, dev[2])
    assert torch.equal(dcode2, dcode) and all(torch.equal(a, g) for a, g in zip(grads2, grads))


def test_single_slice_forward_above_64_kib_of_lds():
    """M = 1 is the one slice count at which the forward asks for more than 64 KiB of dynamic LDS (a whole tile of 256
    points in the point table) and must raise the kernel's limit first; two tiles, the second ragged.  A softmax over one
    slice is expf(0) / 1: exactly one, through the two-coordinate entry and the point-feature entry alike."""
    from transformerbasednavierstokesolver_amd import ops
    code, pos, params, _ = _code_sw_operands(1, 300, 1, 16, seed=6)
    P = tuple(p.cuda() for p in params)
    for fwd in (ops.code_slice_weights_fwd, ops.point_slice_weights_fwd):
        sw = poisoned(fwd, code.cuda(), pos.cuda(), P)
        assert sw.shape == (1, 1, 300, 1) and torch.equal(sw, torch.ones(1, 1, 300, 1, device="cuda"))


def test_code_slice_weights_refusals_and_empty_batch():
    from transformerbasednavierstokesolver_amd import _lib, ops
    lib = _lib.load()
    # pa2d_code_slice_weights_fwd(code, pos, w1, b1, w2, b2, w3, b3, sw, B, N, M, C, hidden, depth, stream, ev0, ev1)
    f = lib.pa2d_code_slice_weights_fwd
    assert f(0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 30, 129, 32, 64, 1, 0, 0, 0) == UNSUP       # M = 129
    assert f(0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 30, 16, 12, 64, 1, 0, 0, 0) == UNSUP        # C = 12
    assert f(0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 30, 16, 32, 128, 1, 0, 0, 0) == UNSUP       # hidden width 128
    assert f(0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 30, 16, 32, 64, 2, 0, 0, 0) == UNSUP        # two hidden layers
    assert f(0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 16, 32, 64, 1, 0, 0, 0) == ARG           # N = 0
    assert f(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 30, 16, 32, 64, 1, 0, 0, 0) == 0            # B = 0
    b = lib.pa2d_code_slice_weights_bwd
    assert b(*([0] * 18), 1, 30, 129, 32, 64, 1, 0, 0, 0, 0) == UNSUP
    assert b(*([0] * 18), 1, 30, 16, 12, 64, 1, 0, 0, 0, 0) == UNSUP
    code, pos, params, _ = _code_sw_operands(1, 30, 16, 32, seed=5)
    wide = (torch.randn(128, 34), torch.randn(128), torch.randn(128, 128), torch.randn(128), torch.randn(1, 128), params[5])
    with pytest.raises(RuntimeError, match="PA2D_ERR_UNSUPPORTED"):
        ops.code_slice_weights_fwd(code.cuda(), pos.cuda(), tuple(p.cuda() for p in wide))
    with pytest.raises(ValueError, match="two point coordinates"):
        ops.code_slice_weights_fwd(code.cuda(), torch.rand(1, 30, 64).cuda(), tuple(p.cuda() for p in params))
    # B = 0: parameter gradients are exact zeros (overwrite) or untouched (accumulate)
    P = tuple(p.cuda() for p in params)
    e_code, e_pos, e_dsw = (torch.empty(0, 16, 32).cuda(), torch.empty(0, 30, 2).cuda(), torch.empty(0, 1, 30, 16).cuda())
    assert ops.code_slice_weights_fwd(e_code, e_pos, P).shape == (0, 1, 30, 16)
    _, *g = ops.code_slice_weights_bwd(e_code, e_pos, P, e_dsw)
    assert all(float(t.abs().sum()) == 0.0 for t in g)
    ones = tuple(torch.ones_like(t) for t in g)
    ops.code_slice_weights_bwd(e_code, e_pos, P, e_dsw, into=ones)
    assert all(bool((t == 1).all()) for t in ones)


# ---------------------------------------------------------------------------------------------- the model against G10
G10 = os.path.join(GOLDEN, "G10_sequensolver.npz")
LAST = "weight_projection.linear_post"
ENGINES = [None, "f32"]          # the default engine (the fp32-accurate split) and exact fp32


@pytest.fixture(scope="module")
def g10():
    return np.load(G10)


def _acceptance(key):
    """forward rel-L2 1e-5, parameter gradients 1e-4, 2e-3 for to_q / to_k, losses at rtol 2e-5."""
    if "loss" in key:
        return 2e-5
    if ".grad." in key:
        return 2e-3 if key.endswith(("to_q.weight", "to_k.weight")) else 1e-4
    return 1e-5


def _bound(g10, key):
    """The acceptance bound, or 4 x the reference's own float32 error where that is more than a quarter of it."""
    base, own = _acceptance(key), float(g10["fp32_self_error." + key])
    return 4 * own if own > base / 4 else base


def _close(g10, key, got, label):
    err, bound = R.golden_rel(g10, key, got), _bound(g10, key)
    print(f"{label} {key}: rel-L2 {err:.3g}, bound {bound:.3g}")
    assert err <= bound, (label, key, err, bound)


def _golden_model(g10, case, engine):
    from transformerbasednavierstokesolver_amd.SequenSolver import SequenSolver
    cfg, geom = json.loads(str(g10[case + ".config"])), json.loads(str(g10["geometry"]))
    sd = {k: torch.from_numpy(v) for k, v in R.golden_state_dict(g10, case).items()}
    enc = {k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}
    m = SequenSolver(enc, T=cfg["T"], layers=cfg["layers"], B=cfg["B"], **geom)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().set_engine(engine)
    return m, tuple(torch.from_numpy(a).cuda() for a in R.golden_inputs(g10, case))


def _loss(out, y):
    from transformerbasednavierstokesolver_amd.utils.testloss import TestLoss
    B = out.shape[0]
    return TestLoss(size_average=False)(out.reshape(B, -1), y.reshape(B, -1))


def _check_grads(g10, pre, m, label):
    none = []
    for k, p in m.named_parameters():
        if p.grad is None:
            none.append(k)
        elif k != LAST + ".bias":          # true gradient 0: judged with its layer's weight, as one tensor
            _close(g10, pre + "grad." + k, p.grad, label)
    assert none == json.loads(str(g10[pre + "no_grad"])), label
    wp = m.weight_projection.linear_post
    if wp.weight.grad is not None:
        _close(g10, pre + f"grad.{LAST}.[weight|bias]", torch.cat((wp.weight.grad.reshape(-1), wp.bias.grad.reshape(-1))), label)


def _zero(m):
    for p in m.parameters():
        p.grad = None


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("case", ["a", "b"])
def test_model_matches_reference(g10, case, engine):
    m, (pos, fx, y, _) = _golden_model(g10, case, engine)
    label = f"G10 {case} engine={engine}"
    # use_gt=True
    out = m(pos, fx, y, use_gt=True)
    for key, got in (("out", out), ("code", m.code), ("slice_weights", m.slice_weights)):
        _close(g10, f"{case}.gt.{key}", got, label)
    assert abs(float(m.slice_weights.sum()) - float(g10[f"{case}.gt.slice_weights.sum"])) < 1e-5 * out.shape[0] * m.N
    assert torch.equal(m.encoder.get_attention_slice(), m.slice_weights)       # the cached weights are those of y
    loss = _loss(out, y)
    _close(g10, f"{case}.gt.loss", loss, label)
    loss.backward()
    _check_grads(g10, f"{case}.gt.", m, label)
    # frame-by-frame encoding gives what the batched encoding gives
    m.batched_encoding = False
    with torch.no_grad():
        out_f = m(pos, fx, y, use_gt=True)
    m.batched_encoding = True
    print(f"{label} batched vs frame-by-frame encoding: rel-L2 {rel_l2(out_f, out):.3g}")
    assert rel_l2(out_f, out) <= 1e-5
    _close(g10, f"{case}.gt.out", out_f, label + " frame by frame")
    _close(g10, f"{case}.gt.slice_weights", m.slice_weights, label + " frame by frame")
    # use_gt=False
    _zero(m)
    out = m(pos, fx, y, use_gt=False)
    for key, got in (("out", out), ("code", m.code), ("slice_weights", m.slice_weights)):
        _close(g10, f"{case}.pred.{key}", got, label)
    assert abs(float(m.slice_weights.sum()) - out.shape[0] * m.N) < 1e-5 * out.shape[0] * m.N
    loss = _loss(out, y)
    _close(g10, f"{case}.pred.loss", loss, label)
    loss.backward()
    _check_grads(g10, f"{case}.pred.", m, label)
    with torch.no_grad():
        _close(g10, f"{case}.get_code", m.get_code(pos, fx, y), label)
        _close(g10, f"{case}.last_slice", m.get_last_slice_weight(pos, fx), label)
    # freeze_attention(): the frozen parameters get no gradient, the others the reference's
    _zero(m)
    m.train()
    m.freeze_attention()
    frozen = [k for k, p in m.named_parameters() if not p.requires_grad and not k.startswith("encoder.")]
    assert frozen == json.loads(str(g10[f"{case}.frozen.names"]))
    loss = _loss(m(pos, fx, y, use_gt=False), y)
    _close(g10, f"{case}.frozen.loss", loss, label)
    loss.backward()
    _check_grads(g10, f"{case}.frozen.", m, label)


@pytest.mark.parametrize("engine", ENGINES)
def test_training_loop_and_rollout_match_reference(g10, engine):
    from transformerbasednavierstokesolver_amd import harness
    from transformerbasednavierstokesolver_amd.optim import FusedAdamW
    hyper = json.loads(str(g10["train.hyper"]))
    label = f"G10 a engine={engine}"
    m, (pos, fx, _, yy) = _golden_model(g10, "a", engine)
    m.eval()
    pred, step_loss, full_loss = harness.sequensolver_rollout(m, pos, fx, yy)
    _close(g10, "a.rollout.pred", pred, label)
    _close(g10, "a.rollout.step_loss", step_loss, label)
    _close(g10, "a.rollout.full_loss", full_loss, label)
    opt = FusedAdamW(m.parameters(), lr=hyper["lr"], weight_decay=hyper["weight_decay"])
    assert not any(p.requires_grad for p in m.encoder.parameters())
    assert len(opt.sync.params) == sum(1 for p in m.parameters() if p.requires_grad)      # the frozen encoder stays out
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=hyper["lr"], epochs=hyper["epochs"],
                                                steps_per_epoch=hyper["steps_per_epoch"])
    losses = []
    for _ in range(hyper["steps"]):
        m.train()
        loss, _ = harness.sequensolver_train_step(m, opt, sched, pos, fx, yy, grad_sync=opt.sync)
        losses.append(float(loss))
    want = g10["a.train.losses"]
    rtol = _bound(g10, "a.train.losses")
    print(f"{label} training losses {losses} against {want.tolist()}, rtol {rtol:.3g}")
    np.testing.assert_allclose(losses, want, rtol=rtol)
    # after freeze_attention() a new optimizer holds the remaining parameters only, and the step still runs
    m.freeze_attention()
    opt2 = FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-5)
    assert len(opt2.sync.params) == sum(1 for k, _ in m.named_parameters() if not k.startswith("encoder.")) - 11 == 18
    before = m.to_q.weight.detach().clone()
    loss, _ = harness.sequensolver_train_step(m, opt2, None, pos, fx, yy, use_gt=False, grad_sync=opt2.sync)
    assert torch.isfinite(loss) and torch.equal(m.to_q.weight, before)


# ---------------------------------------------------------------------------------------------- a shape off the reference's
TINY_ENCODER = dict(space_dim=2, n_layers=2, n_hidden=16, n_head=1, slice_num=8, fun_dim=1, out_dim=1, mlp_ratio=1,
                    unified_pos=0, H=6, W=5)


def _tiny_restated(sd, dtype, x, fx, y, use_gt):
    sd = {k: v.to(dtype).clone().requires_grad_(not k.startswith("encoder.")) for k, v in sd.items()}
    out, code, sw = R.forward(sd, TINY_ENCODER, 2, x.to(dtype), fx.to(dtype), y.to(dtype), use_gt=use_gt)
    B = out.shape[0]
    yd = y.to(dtype)
    loss = (torch.linalg.vector_norm((out - yd).reshape(B, -1), dim=1) / torch.linalg.vector_norm(yd.reshape(B, -1), dim=1)).sum()
    loss.backward()
    res = {"out": out.detach(), "code": code.detach(), "slice_weights": sw.detach(), "loss": loss.detach()}
    res.update({"grad." + k: v.grad for k, v in sd.items() if v.grad is not None and k != LAST + ".bias"})
    if sd[LAST + ".weight"].grad is not None:
        res[f"grad.{LAST}.[weight|bias]"] = torch.cat((sd[LAST + ".weight"].grad.reshape(-1), sd[LAST + ".bias"].grad.reshape(-1)))
    return res


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("use_gt", [True, False])
def test_tiny_model_off_the_reference_shape(use_gt, engine):
    """6 x 5 mesh, C=16, M=8, T=2, B=3 through `encoder_config`, against the float64 restatement; bounds as for G10, with
    the float32 CPU restatement in the role of the fixture's self error."""
    from transformerbasednavierstokesolver_amd.SequenSolver import SequenSolver
    torch.manual_seed(7)
    m = SequenSolver(None, T=2, W=5, H=6, M=8, C=16, B=3, layers=2, encoder_config=TINY_ENCODER)
    with torch.no_grad():      # spread the predicted slice weights, and give every parameter a non-trivial value
        for k, p in m.named_parameters():
            if k.endswith(".bias") or k.startswith("ln_"):
                p.add_(0.1 * torch.randn_like(p))
        m.weight_projection.linear_post.weight.mul_(4.0)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(8)
    x, fx, y = torch.rand(3, 30, 2, generator=g), torch.randn(3, 30, 2, generator=g), torch.randn(3, 30, 1, generator=g)
    r64 = _tiny_restated(sd, torch.float64, x, fx, y, use_gt)
    r32 = _tiny_restated(sd, torch.float32, x, fx, y, use_gt)
    m = m.cuda().set_engine(engine)
    out = m(x.cuda(), fx.cuda(), y.cuda(), use_gt=use_gt)
    loss = _loss(out, y.cuda())
    loss.backward()
    got = {"out": out, "code": m.code, "slice_weights": m.slice_weights, "loss": loss}
    got.update({"grad." + k: p.grad for k, p in m.named_parameters() if p.grad is not None and k != LAST + ".bias"})
    if not use_gt:
        wp = m.weight_projection.linear_post
        got[f"grad.{LAST}.[weight|bias]"] = torch.cat((wp.weight.grad.reshape(-1), wp.bias.grad.reshape(-1)))
    assert sorted(got) == sorted(r64)
    for k, want in r64.items():
        base, own = _acceptance("." + k), rel_l2(r32[k], want)
        bound = 4 * own if own > base / 4 else base
        err = rel_l2(got[k], want)
        print(f"tiny use_gt={use_gt} engine={engine} {k}: rel-L2 {err:.3g}, bound {bound:.3g}")
        assert err <= bound, (k, err, bound)
