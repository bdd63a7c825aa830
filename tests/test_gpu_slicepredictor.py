"""The conv slice predictors on the MI355X: the single 3x3 conv, the whole-tensor z-score and the wide slice-weight stage
element by element / row by row against float64, then SliceLearner and VorticitySliceLearner against the float64
restatement (tests/slicepredictor_restatement.py) and against the reference's results in tests/golden/G12_slicepredictor.npz
(written by tools/make_golden_slicepredictor.py).

Bounds.  The single conv takes the per-element bounds of the pair (elementwise_check.TAU, "fwd" for the forward and the data
gradient, "wgrad" for the weight and bias gradients, per engine) with the same check_products scales.  The z-score and the
wide slice weights have no calibrated entry, so the rule of test_gpu_learnslice.py applies: the yardstick is the same
restatement evaluated by torch in float32 on the CPU against its float64 result on the test's own inputs, and the bound is
4 x its worst row error; every test prints the measured GPU value beside the bound before it asserts.  Against G12 the
yardstick of the slice weights and the loss is the reference's own float32 run, stored beside its float64 run; G12 holds the
gradients in float64 only, so their yardstick is the float32 restatement again.

dt of the wide stage is ONE number, so the rule gives it the error of one float32 evaluation and no worst over rows; see
_dt_dsw for the dsw that keeps that number well conditioned.

Measured on one MI355X box (worst GPU value / its bound, at the case where the ratio is largest):

  conv3x3   forward 3.33e-07, data gradient 3.15e-07 / 1.6e-06 (1x64x64x256, f32); dw 2.17e-07, db 3.95e-08 / 1e-06; the split
            engine at 1x64x64x256: 2.76e-07, 2.82e-07, 2.63e-08, 9.35e-09
  zscore    y 3.07e-08 / 1.96e-07, dx 2.95e-08 / 2.18e-07 (4099 x 256; y 3.61e-08 / 1.74e-05 at mean = 100 std); mu to 1e-12
            and sigma to 1e-9 of float64 everywhere; exact zeros and sigma = 0 for constant inputs
  wide_sw   sw 9.33e-07 / 3.61e-06 (60 x 32 x 12, pitch 48), dx 2.64e-06 / 8.94e-06 (60 x 512 x 128), dws 2.99e-06 / 1.08e-05
            (60 x 32 x 12, t = 0.05), dbs 1.10e-07 / 3.99e-07 (257 x 256 x 16, t = 7), dt 5.89e-08 / 5.89e-07 (60 x 512 x 128;
            4.59e-09 / 4.10e-07 at 4099 x 384 x 16)
  modules   SliceLearner 6x5: sw 1.66e-06 / 5.88e-06, worst gradients temperature 3.49e-07 / 6.01e-07 (unified_pos, fx=None)
            and preprocess.linear_post.weight 4.54e-06 / 9.35e-06 (fx=None); VorticitySliceLearner 6x5 B=2: sw 1.20e-06 /
            4.97e-06, worst gradient in_project_slice.linears.0.0.bias 8.23e-07 / 3.86e-06, dcode 2.06e-06 / 6.72e-06; against
            G12 at 64 x 64: sw 7.01e-06 / 1.37e-05 (no code, f32), 2.81e-06 / 1.48e-05 (code); the f32 and split engines
            give the same bits at the 6x5 sizes; rollout of 3 steps 2.05e-06 / 7.18e-06
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from elementwise_check import TAU, check_products, check_rows, poisoned
import slicepredictor_restatement as R
from test_gpu_sequensolver import _bounded, _row_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G12 = os.path.join(GOLDEN, "G12_slicepredictor.npz")


@pytest.fixture(scope="module")
def g12():
    return np.load(G12)


def _cuda(*ts):
    return [None if t is None else torch.as_tensor(t).to(DEV) for t in ts]


# ---------------------------------------------------------------------------------------------- single 3x3 conv
def _conv64(x, w, b, H, W):
    """Zero-padded 3x3 cross-correlation as nine shifted GEMMs: fp64 on the device."""
    B, N, C = x.shape
    xp = F.pad(x.reshape(B, H, W, C), (0, 0, 1, 1, 1, 1))
    out = b.expand(B, H, W, w.shape[0])
    for ky in range(3):
        for kx in range(3):
            out = out + xp[:, ky:ky + H, kx:kx + W, :] @ w[:, :, ky, kx].t()
    return out.reshape(B, N, -1)


def _conv_refs(x, w, b, dout, H, W):
    def run(x, w, b, dout):
        ts = [t.detach().clone().requires_grad_(True) for t in (x, w, b)]
        out = _conv64(ts[0], ts[1], ts[2], H, W)
        out.backward(dout)
        return (out.detach(),) + tuple(t.grad for t in ts)
    return run(x, w, b, dout), run(x.abs(), w.abs(), b.abs(), dout.abs())


@pytest.mark.parametrize("B,H,W,C", [(1, 5, 7, 16), (2, 6, 5, 32), (1, 64, 64, 256)])
def test_conv3x3_elementwise(B, H, W, C):
    from transformerbasednavierstokesolver_amd import ops
    rng = np.random.default_rng(B * H + W + C)
    r = lambda *s, scale=1.0: torch.from_numpy((rng.standard_normal(s) * scale).astype(np.float32)).to(DEV)
    N = H * W
    x, dout, w, b = r(B, N, C), r(B, N, C), r(C, C, 3, 3, scale=(9 * C) ** -0.5), 0.1 * r(C)
    (out_r, dx_r, dw_r, db_r), (out_s, dx_s, dw_s, db_s) = _conv_refs(x.double(), w.double(), b.double(), dout.double(), H, W)
    for engine in ("f32", "split"):
        tag = f"[{engine}] conv3x3 B={B} H={H} W={W} C={C}"
        tf, tw = TAU[(engine, "fwd")], TAU[(engine, "wgrad")]
        out = poisoned(ops.conv3x3_fwd, x, w, b, H, W, engine=engine)
        v = [check_products(out, out_r, out_s, tf, hw=(H, W), label=tag + " forward")]
        dxn, dw, db = poisoned(ops.conv3x3_bwd, dout, x, w, H, W, engine=engine)
        v.append(check_products(dxn, dx_r, dx_s, tf, hw=(H, W), label=tag + " data gradient"))
        v.append(check_products(dw.reshape(C, -1), dw_r.reshape(C, -1), dw_s.reshape(C, -1), tw, label=tag + " dw [co, ci*9+tap]"))
        v.append(check_products(db, db_r, db_s, tw, label=tag + " db"))
        print(f"{tag}: |err|/scale forward {v[0]:.3g}, data gradient {v[1]:.3g} (bound {tf:.3g}); dw {v[2]:.3g}, db {v[3]:.3g} "
              f"(bound {tw:.3g})")
        # a prepacked call (packs made once inside a weights_frozen scope) gives the same bits
        with ops.weights_frozen() as scope:
            assert torch.equal(ops.conv3x3_fwd(x, w, b, H, W, engine=engine), out)
            dxp, dwp, dbp = ops.conv3x3_bwd(dout, x, w, H, W, engine=engine)
            assert len(scope.packs1) == 2 and not scope.packs
            scope.refresh()
            assert torch.equal(ops.conv3x3_fwd(x, w, b, H, W, engine=engine), out)
        assert torch.equal(dxp, dxn) and torch.equal(dwp, dw) and torch.equal(dbp, db)
        # dxn = NULL: the parameter gradients alone, the same bits
        none, dw0, db0 = ops.conv3x3_bwd(dout, x, w, H, W, need_dx=False, engine=engine)
        assert none is None and torch.equal(dw0, dw) and torch.equal(db0, db)
        # accumulate = 1: into zeros the same bits, into the result exactly twice it
        zeros = (torch.zeros_like(dw), torch.zeros_like(db))
        ops.conv3x3_bwd(dout, x, w, H, W, engine=engine, into=zeros)
        assert torch.equal(zeros[0], dw) and torch.equal(zeros[1], db)
        twice = (dw.clone(), db.clone())
        ops.conv3x3_bwd(dout, x, w, H, W, engine=engine, into=twice)
        assert torch.equal(twice[0], 2 * dw) and torch.equal(twice[1], 2 * db)


def test_conv3x3_refusals_and_empty_batch():
    from transformerbasednavierstokesolver_amd import ops
    x, w, b = torch.zeros(1, 12, 24, device=DEV), torch.zeros(24, 24, 3, 3, device=DEV), torch.zeros(24, device=DEV)
    with pytest.raises(RuntimeError, match="1002"):
        ops.conv3x3_fwd(x, w, b, 3, 4)                                  # C % 16 != 0
    with pytest.raises(ValueError):
        ops.conv3x3_fwd(x, w, b, 3, 4, engine="bf16s")
    x0, w, b = torch.zeros(0, 12, 32, device=DEV), torch.ones(32, 32, 3, 3, device=DEV), torch.ones(32, device=DEV)
    assert ops.conv3x3_fwd(x0, w, b, 3, 4).shape == (0, 12, 32)
    dxn, dw, db = ops.conv3x3_bwd(x0, x0, w, 3, 4)
    assert dxn.shape == (0, 12, 32) and float(dw.abs().max()) == 0 and float(db.abs().max()) == 0
    keep = (torch.ones_like(dw), torch.ones_like(db))
    ops.conv3x3_bwd(x0, x0, w, 3, 4, into=keep)
    assert float(keep[0].min()) == 1 and float(keep[1].min()) == 1


# ---------------------------------------------------------------------------------------------- z-score
ZSCORE_CASES = [      # rows, C, pitch, offset of the data in units of its std
    (1, 4, 4, 0.0), (30, 32, 64, 0.0), (4099, 256, 256, 0.0), (257, 64, 64, 100.0), (30, 32, 64, 100.0),
]


@pytest.mark.parametrize("rows,C,pitch,offset", ZSCORE_CASES)
def test_zscore_forward_backward_rows(rows, C, pitch, offset):
    from transformerbasednavierstokesolver_amd import ops
    g = torch.Generator().manual_seed(5000 + rows + C + pitch)
    buf = torch.randn(rows, pitch, generator=g) * 0.7 + offset * 0.7
    dbuf = torch.randn(rows, pitch, generator=g)
    x, dy = buf[:, :C], dbuf[:, :C]

    def restated(dtype):
        xx = x.to(dtype).clone().requires_grad_(True)
        y = R.zscore(xx)
        y.backward(dy.to(dtype))
        return y.detach(), xx.grad, xx.detach().mean(), xx.detach().std(unbiased=False)

    y64, dx64, mu64, sd64 = restated(torch.float64)
    y32, dx32, _, _ = restated(torch.float32)
    xd, dyd = buf.to(DEV)[:, :C], dbuf.to(DEV)[:, :C]          # column views of pitch `pitch`
    label = f"zscore rows={rows} C={C} pitch={pitch} mean={offset:g} std"
    y, stats = poisoned(ops.zscore_fwd, xd)
    assert y.is_contiguous() and stats.dtype == torch.float64
    print(f"{label}: mu {float(stats[0]):.9g} (fp64 {float(mu64):.9g}), sigma {float(stats[1]):.9g} (fp64 {float(sd64):.9g})")
    assert abs(float(stats[0]) - float(mu64)) <= 1e-12 * max(1.0, abs(float(mu64)))
    assert abs(float(stats[1]) - float(sd64)) <= 1e-9 * float(sd64)      # E[x^2] - mu^2 in fp64 at mean = 100 std: 1e-12 * 1e4
    _bounded("y", y, y64, y32, label)
    dx = poisoned(ops.zscore_bwd, dyd, y, stats)
    _bounded("dx", dx, dx64, dx32, label)
    # the closed form against autograd, both in float64 (what the kernel evaluates is the derivative)
    assert R.rel(R.zscore_backward(dy.double(), y64, sd64), dx64) < 1e-9
    # the autograd node: same bits as the two ops
    xa = xd.clone().requires_grad_(True)
    from transformerbasednavierstokesolver_amd import functional as Fn
    ya = Fn.zscore(xa)
    ya.backward(dyd)
    assert torch.equal(ya.detach(), y) and torch.equal(xa.grad, dx)


def test_zscore_constant_input_and_refusals():
    from transformerbasednavierstokesolver_amd import ops
    for shape, value in (((4099, 256), 3.14159), ((1, 4), -2.5e6), ((30, 32), 0.0)):
        y, stats = poisoned(ops.zscore_fwd, torch.full(shape, value, device=DEV))
        assert float(y.abs().max()) == 0.0 and float(stats[0]) == float(np.float32(value)), (shape, value)
        assert float(stats[1]) == 0.0, (shape, value, float(stats[1]))
    with pytest.raises(RuntimeError, match="1002"):
        ops.zscore_fwd(torch.zeros(5, 6, device=DEV))                   # C % 4 != 0
    y, stats = ops.zscore_fwd(torch.zeros(0, 8, device=DEV))            # rows = 0: a no-op
    assert y.shape == (0, 8)


def test_zscore_node_takes_any_layout():
    """A gradient without a row pitch (expanded by sum()) and an input whose rows sit at no one pitch (a transpose): the node
    copies them, and the results are those of the contiguous tensors."""
    from transformerbasednavierstokesolver_amd import functional as Fn
    g = torch.Generator().manual_seed(77)
    x = torch.randn(2, 6, 8, generator=g).to(DEV)
    xt = x.transpose(0, 1)                                              # [6, 2, 8], strides (8, 48, 1)
    a = xt.clone().requires_grad_(True)                                 # clone keeps the strides
    assert not a.is_contiguous()
    ya = Fn.zscore(a)
    ya.sum().backward()
    b = xt.contiguous().requires_grad_(True)
    yb = Fn.zscore(b)
    yb.backward(torch.ones_like(yb))
    assert torch.equal(ya, yb) and torch.equal(a.grad, b.grad)
    assert float(b.grad.abs().max()) < 1e-5                             # d sum(y) / dx = 0: y sums to zero whatever x


# ---------------------------------------------------------------------------------------------- wide slice weights
WIDE_CASES = [      # rows, D, M, t, pitch of x (0 = contiguous)
    (1, 16, 1, 0.5, 0), (60, 32, 12, 0.5, 48), (257, 256, 16, 0.5, 0), (4099, 384, 16, 0.5, 0), (60, 512, 128, 0.5, 0),
    (257, 64, 100, 0.5, 0), (60, 32, 12, 0.05, 0), (60, 32, 12, 7.0, 0), (257, 256, 16, 0.05, 0), (257, 256, 16, 7.0, 0),
]


def _wide_operands(rows, D, M, t, pitch, seed):
    g = torch.Generator().manual_seed(seed)
    buf = torch.randn(rows, pitch or D, generator=g)
    ws = torch.randn(M, D, generator=g) * (1.5 / D ** 0.5)
    bs = torch.randn(M, generator=g) * 0.1
    dsw = torch.randn(rows, M, generator=g)
    return buf, ws, bs, torch.tensor([t]), dsw


def _dt_dsw(x, ws, bs, dsw):
    """The dsw under which dt is checked: the normal noise plus the logits.  dt = -(1/t^2) sum_rows Cov_sw(dsw, logit) is ONE
    number.  With noise alone the rows' terms have either sign and the sum cancels to 1/45 .. 1/1700 of sum |dl * logit| at
    these shapes (in float64), so ANY float32 evaluation misses it by that factor times 1e-7, and by how much is luck: no
    yardstick.  The logit part adds Var_sw(logit) >= 0 to every row's term (a loss that rewards the larger logit, as a
    trained one does), the sum keeps a quarter of sum |dl * logit|, and the rule's one float32 evaluation bounds it.  dx, dws
    and dbs are per row and keep the plain noise."""
    return dsw + (x @ ws.t() + bs)


def _wide_restated(x, ws, bs, temp, dsw, dtype):
    ts = [t.to(dtype).clone().requires_grad_(True) for t in (x, ws, bs, temp)]
    sw = R.wide_slice_weights(*ts)
    sw.backward(dsw.to(dtype))
    return (sw.detach(),) + tuple(t.grad for t in ts)


@pytest.mark.parametrize("rows,D,M,t,pitch", WIDE_CASES)
def test_wide_slice_weights_forward_backward_rows(rows, D, M, t, pitch):
    from transformerbasednavierstokesolver_amd import ops
    buf, ws, bs, temp, dsw = _wide_operands(rows, D, M, t, pitch, seed=6000 + rows + D + M + int(10 * t))
    x = buf[:, :D]
    r64 = _wide_restated(x, ws, bs, temp, dsw, torch.float64)
    r32 = _wide_restated(x, ws, bs, temp, dsw, torch.float32)
    xd = buf.to(DEV)[:, :D]
    wsd, bsd, td, dswd = _cuda(ws, bs, temp, dsw)
    label = f"wide_sw rows={rows} D={D} M={M} t={t:g} pitch={pitch or D}"
    sw = poisoned(ops.wide_slice_weights_fwd, xd, wsd, bsd, td)
    assert sw.shape == (rows, M)
    _bounded("sw", sw, r64[0], r32[0], label)
    assert float((sw.sum(-1) - 1).abs().max()) < 1e-5
    dx, dws, dbs, dt = poisoned(ops.wide_slice_weights_bwd, xd, wsd, bsd, td, dswd)
    clamped = t < 0.1 or t > 5
    if M > 1:      # one slice: the weight is 1 whatever the operands, every gradient is exactly zero
        _bounded("dx", dx, r64[1], r32[1], label)
        _bounded("dws", dws, r64[2], r32[2], label)
        _bounded("dbs", dbs, r64[3], r32[3], label)
        if not clamped:
            dsw_t = _dt_dsw(x, ws, bs, dsw)
            t64, t32 = (_wide_restated(x, ws, bs, temp, dsw_t, dtype)[4] for dtype in (torch.float64, torch.float32))
            dt_t = poisoned(ops.wide_slice_weights_bwd, xd, wsd, bsd, td, dsw_t.to(DEV), need_dx=False)[3]
            _bounded("dt", dt_t, t64, t32, label)
    else:
        assert all(float(g.abs().max()) == 0 for g in (dx, dws, dbs, dt))
    if clamped:
        assert float(dt) == 0.0 and float(r64[4]) == 0.0
    # no dx on request, accumulate into zeros / into the result, a second run: the same bits
    grads = (dws, dbs, dt)
    zeros = tuple(torch.zeros_like(g) for g in grads)
    none, *acc0 = ops.wide_slice_weights_bwd(xd, wsd, bsd, td, dswd, need_dx=False, into=zeros)
    assert none is None and all(torch.equal(a, g) for a, g in zip(acc0, grads))
    twice = tuple(g.clone() for g in grads)
    ops.wide_slice_weights_bwd(xd, wsd, bsd, td, dswd, into=twice)
    assert all(torch.equal(a, 2 * g) for a, g in zip(twice, grads))
    assert torch.equal(ops.wide_slice_weights_fwd(xd, wsd, bsd, td), sw)


def test_wide_slice_weights_refusals_and_empty_batch():
    from transformerbasednavierstokesolver_amd import ops
    z = lambda *s: torch.zeros(*s, device=DEV)
    for D, M in ((12, 4), (516, 4), (32, 129)):
        with pytest.raises(RuntimeError, match="1002"):
            ops.wide_slice_weights_fwd(z(8, D), z(M, D), z(M), z(1) + 0.5)
        with pytest.raises(RuntimeError, match="1002"):
            ops.wide_slice_weights_bwd(z(8, D), z(M, D), z(M), z(1) + 0.5, z(8, M))
    assert ops.wide_slice_weights_fwd(z(0, 32), z(12, 32), z(12), z(1) + 0.5).shape == (0, 12)
    dx, dws, dbs, dt = ops.wide_slice_weights_bwd(z(0, 32), z(12, 32), z(12), z(1) + 0.5, z(0, 12))
    assert dx.shape == (0, 32) and all(float(g.abs().max()) == 0 for g in (dws, dbs, dt))
    keep = (z(12, 32) + 1, z(12) + 1, z(1) + 1)
    ops.wide_slice_weights_bwd(z(0, 32), z(12, 32), z(12), z(1) + 0.5, z(0, 12), into=keep)
    assert all(float(k.min()) == 1 for k in keep)


# ---------------------------------------------------------------------------------------------- modules
def _load(module, sd):
    res = module.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return module.to(DEV)


def _restated_grads(fn, sd, inputs, dsw, dtype, code_index=None):
    """sw and the gradients of sum(sw * dsw) (parameters that the forward reads, and the input `code_index`)."""
    P = R.to_torch(sd, dtype, requires_grad=True)
    ins = [None if a is None else torch.as_tensor(a).to(dtype) for a in inputs]
    if code_index is not None:
        ins[code_index].requires_grad_(True)
    sw = fn(P, *ins)
    (sw * torch.as_tensor(dsw).to(dtype)).sum().backward()
    grads = {k: p.grad for k, p in P.items() if p.grad is not None}
    return sw.detach(), grads, (ins[code_index].grad if code_index is not None else None)


def _check_module(label, module, sw, sd, r64, r32, dcode=None):
    _bounded("sw", sw, r64[0], r32[0], label)
    got = {k: p.grad for k, p in module.named_parameters() if p.grad is not None}
    assert sorted(got) == sorted(r64[1]), (sorted(got), sorted(r64[1]))
    for k in got:      # conv kernels as [co, ci*9+tap] rows, like the pair's element-wise test
        shp = (got[k].shape[0], -1) if got[k].dim() == 4 and got[k].shape[0] > 1 else got[k].shape
        _bounded(f"d {k}", got[k].reshape(shp), r64[1][k].reshape(shp), r32[1][k].reshape(shp), label)
    if dcode is not None:
        _bounded("dcode", dcode, r64[2], r32[2], label)


@pytest.mark.parametrize("engine", ["f32", "split"])
def test_slicelearner_against_restatement_and_g12(g12, engine):
    from transformerbasednavierstokesolver_amd.SliceLearner import SliceLearner
    sd, x, fx, dsw = R.small_case()
    R.check_sums(g12, "small", sd, (x, fx, dsw))
    H, W = R.SMALL["H"], R.SMALL["W"]
    fn = lambda P, a, b: R.slice_learner(P, a, b, H, W)
    r64 = _restated_grads(fn, sd, (x, fx), dsw, torch.float64)
    r32 = _restated_grads(fn, sd, (x, fx), dsw, torch.float32)
    m = _load(SliceLearner(**R.SMALL), sd).set_engine(engine)
    xd, fxd, dswd = _cuda(x, fx, dsw)
    sw = m(xd, fxd)
    assert sw.shape == (R.SMALL_B, 1, H * W, R.SMALL["slice_num"])
    (sw * dswd).sum().backward()
    label = f"[{engine}] SliceLearner 6x5 n_hidden=32 M=12 B=2"
    _check_module(label, m, sw, sd, r64, r32)
    # against the reference itself: its float64 run, within 4 x its own float32 run
    tol = 4 * _row_err(torch.from_numpy(g12["small.sw.f32"]), torch.from_numpy(g12["small.sw.f64"]))
    worst = check_rows(sw.reshape(-1, 12), torch.from_numpy(g12["small.sw.f64"]).reshape(-1, 12), tol, label=label + " vs G12")
    print(f"{label} vs G12: worst row rel-L2 {worst:.3g}, bound {tol:.3g}")
    for k, p in m.named_parameters():
        if p.grad is not None:
            assert R.rel(p.grad, g12[f"small.grad.{k}"]) < 4 * max(R.rel(r32[1][k], r64[1][k]), 1e-7), k


@pytest.mark.parametrize("unified_pos,with_fx", [(False, False), (True, True), (True, False)])
def test_slicelearner_placeholder_and_unified_pos(unified_pos, with_fx):
    from transformerbasednavierstokesolver_amd.SliceLearner import SliceLearner
    cfg = dict(space_dim=2, n_hidden=32, fun_dim=3 if with_fx else 0, ref=4, unified_pos=unified_pos, H=6, W=5, slice_num=12)
    sd = R.draw_state(R.slice_learner_shapes(**{k: v for k, v in cfg.items() if k not in ("H", "W")}), 81 + unified_pos, 0.4)
    x, fx, _, dsw, _ = R.draw_inputs(181, 2, 30, 2, 3, 12, 1)
    fx = fx if with_fx else None
    m = _load(SliceLearner(**cfg), sd)
    pos = m.pos.detach().cpu().reshape(1, 30, 16) if unified_pos else None
    fn = lambda P, a, b: R.slice_learner(P, a, b, 6, 5, pos=None if pos is None else pos.to(a.dtype))
    r64 = _restated_grads(fn, sd, (x, fx), dsw, torch.float64)
    r32 = _restated_grads(fn, sd, (x, fx), dsw, torch.float32)
    xd, fxd, dswd = _cuda(x, fx, dsw)
    sw = m(xd, fxd)
    (sw * dswd).sum().backward()
    assert (m.placeholder.grad is not None) == (not with_fx)
    _check_module(f"SliceLearner unified_pos={unified_pos} fx={'given' if with_fx else 'None'}", m, sw, sd, r64, r32)


@pytest.mark.parametrize("engine", ["f32", "split"])
def test_vorticity_learner_small_against_restatement(engine):
    """6 x 5, n_hidden 32, M 12, B 2: the z-scores couple the two samples; the code gets its gradient."""
    from transformerbasednavierstokesolver_amd.SliceLearner import VorticitySliceLearner
    cfg = dict(C=8, M=12, T=10, H=6, W=5, n_hidden=32)
    sd = R.draw_state(R.vorticity_shapes(1, True, 8, 12, 10, 32), 91, 0.5)
    x, fx, code, dsw, _ = R.draw_inputs(191, 2, 30, 64, 10, 12, 8)
    fn = lambda P, a, b, c: R.vorticity_learner(P, a, b, c, 6, 5)
    r64 = _restated_grads(fn, sd, (x, fx, code), dsw, torch.float64, code_index=2)
    r32 = _restated_grads(fn, sd, (x, fx, code), dsw, torch.float32, code_index=2)
    m = _load(VorticitySliceLearner(1, True, **cfg), sd).set_engine(engine)
    xd, fxd, cd, dswd = _cuda(x, fx, code, dsw)
    cd.requires_grad_(True)
    sw = m(xd, fxd, cd)
    assert sw.shape == (2, 1, 30, 12)
    (sw * dswd).sum().backward()
    _check_module(f"[{engine}] VorticitySliceLearner 6x5 n_hidden=32 M=12 C=8 B=2", m, sw, sd, r64, r32, dcode=cd.grad)
    # a code that needs no gradient: the same weights and parameter gradients, nothing for the code
    m.zero_grad(set_to_none=True)
    c2 = cd.detach().clone()
    sw2 = m.forward_from_vorticity(xd, fxd, c2)
    (sw2 * dswd).sum().backward()
    assert torch.equal(sw2, sw) and c2.grad is None


_VORT_REFS = {}


def _vort_refs(name):
    """float64 / float32 restatement of a G12 case with the gradients of its loss, computed once."""
    if name not in _VORT_REFS:
        sd, x, fx, code, target = R.vort_case(name)
        res = {}
        for dtype in (torch.float64, torch.float32):
            P = R.to_torch(sd, dtype, requires_grad=True)
            c = None if code is None else torch.from_numpy(code).to(dtype)
            sw = R.vorticity_learner(P, torch.from_numpy(x).to(dtype), torch.from_numpy(fx).to(dtype), c, 64, 64)
            loss = F.mse_loss(sw, torch.from_numpy(target).to(dtype))
            loss.backward()
            res[dtype] = (sw.detach(), float(loss.detach()), {k: p.grad for k, p in P.items()})
        _VORT_REFS[name] = (sd, x, fx, code, target, res)
    return _VORT_REFS[name]


@pytest.mark.parametrize("engine", ["f32", "split"])
@pytest.mark.parametrize("name", list(R.VORT_CASES))
def test_vorticity_learner_against_g12(g12, name, engine):
    from transformerbasednavierstokesolver_amd.SliceLearner import VorticitySliceLearner
    sd, x, fx, code, target, res = _vort_refs(name)
    R.check_sums(g12, f"vort.{name}", sd, (x, fx, code, target))
    m = _load(VorticitySliceLearner(1, R.VORT_CASES[name]["use_code"]), sd).set_engine(engine)
    xd, fxd, cd, td = _cuda(x, fx, code, target.astype(np.float32))
    sw = m(xd, fxd, cd)
    loss = F.mse_loss(sw, td)
    loss.backward()
    label = f"[{engine}] VorticitySliceLearner G12 {name}"
    key = f"vort.{name}"
    tol = 4 * _row_err(torch.from_numpy(g12[key + ".sw.f32"]), torch.from_numpy(g12[key + ".sw.f64"]))
    worst = check_rows(sw[0, 0, ::R.STRIDE], torch.from_numpy(g12[key + ".sw.f64"]), tol, label=label + " sw")
    print(f"{label} sw: worst row rel-L2 {worst:.3g}, bound {tol:.3g} (the reference's float32 run)")
    ltol = 4 * abs(float(g12[key + ".loss.f32"]) - float(g12[key + ".loss.f64"]))
    lerr = abs(float(loss.detach()) - float(g12[key + ".loss.f64"]))
    print(f"{label} loss: |err| {lerr:.3g}, bound {ltol:.3g}")
    assert lerr <= ltol
    g64, g32 = res[torch.float64][2], res[torch.float32][2]
    for k, p in m.named_parameters():
        n32, s32 = R.grad_sample(g32[k].numpy())
        n, s = R.grad_sample(p.grad.cpu().numpy())
        gtol = 4 * R.rel(s32, g12[f"{key}.grad.{k}.sample"])
        err = R.rel(s, g12[f"{key}.grad.{k}.sample"])
        print(f"{label} d {k}: sample rel-L2 {err:.3g}, bound {gtol:.3g}; norm {n:.6g} (fp64 {float(g12[f'{key}.grad.{k}.norm']):.6g})")
        assert err <= gtol, k
        assert abs(n - float(g12[f"{key}.grad.{k}.norm"])) <= gtol * n, k


# ---------------------------------------------------------------------------------------------- train step and rollout
TINY = dict(T=2, W=5, H=6, M=8, C=16, layers=2)
HYPER = dict(lr=1e-3, weight_decay=1e-5)


def _tiny_setup(kind, seed):
    """(frozen tiny SequenSolver on the CPU, predictor factory, predictor state_dict, restated forward, x, fx, yy)."""
    import sequensolver_restatement as S
    from test_sequensolver_host import TINY_ENCODER
    from transformerbasednavierstokesolver_amd.SequenSolver import SequenSolver
    from transformerbasednavierstokesolver_amd.SliceLearner import SliceLearner, VorticitySliceLearner
    torch.manual_seed(seed)
    seq = SequenSolver(None, B=3, encoder_config=TINY_ENCODER, **TINY)
    if kind == "vorticity":
        make = lambda: VorticitySliceLearner(0, True, C=16, M=8, T=2, H=6, W=5, n_hidden=32)
        shapes, fwd = R.vorticity_shapes(0, True, 16, 8, 2, 32), (lambda P, x, fx, code: R.vorticity_learner(P, x, fx, code, 6, 5))
    else:
        make = lambda: SliceLearner(space_dim=2, n_hidden=32, fun_dim=2, H=6, W=5, slice_num=8)
        shapes = R.slice_learner_shapes(space_dim=2, n_hidden=32, fun_dim=2, slice_num=8)
        fwd = lambda P, x, fx, code: R.slice_learner(P, x, fx, 6, 5)
    sd = R.draw_state(shapes, seed + 1, 0.5)
    g = torch.Generator().manual_seed(seed + 2)
    x, fx, yy = torch.rand(3, 30, 2, generator=g), torch.randn(3, 30, 2, generator=g), torch.randn(3, 30, 2, generator=g)

    def code_and_target(sd_seq, x, fx, y):
        enc, own = S.split_state_dict(sd_seq)
        B, T = fx.shape[0], fx.shape[2]
        with torch.no_grad():
            target = None if y is None else S.encode(enc, TINY_ENCODER, x, y)[1]
            codes = [S.encode(enc, TINY_ENCODER, x, fx[:, :, i:i + 1])[0] for i in range(T)]
            tokens = torch.stack([c.reshape(B, -1) for c in codes], 1)
            code = S.tokens_to_code(own, tokens, 2, tokens.shape[-1] ** -0.5).reshape(B, 1, 8, 16)
        return code, target

    return seq, make, sd, fwd, code_and_target, x, fx, yy


def _restated_train_step(sd_seq, sd, fwd, code_and_target, x, fx, yy, dtype):
    """LearnSlice.py:929-962 in `dtype` with torch.optim.AdamW: (summed loss, parameters after the one step)."""
    seq = {k: v.to(dtype) for k, v in sd_seq.items()}
    P = R.to_torch(sd, dtype, requires_grad=True)
    opt = torch.optim.AdamW(list(P.values()), **HYPER)
    x, fx, yy = x.to(dtype), fx.to(dtype), yy.to(dtype)
    loss = 0
    for t in range(yy.shape[-1]):
        y = yy[..., t:t + 1]
        code, target = code_and_target(seq, x, fx, y)
        loss = loss + F.mse_loss(fwd(P, x, fx, code), target)
        fx = torch.cat((fx[..., 1:], y), dim=-1)
    opt.zero_grad()
    loss.backward()
    opt.step()
    return float(loss.detach()), {k: v.detach() for k, v in P.items()}, {k: v.grad is not None for k, v in P.items()}


@pytest.mark.parametrize("kind", ["vorticity", "slicelearner"])
def test_slice_predictor_train_step_on_a_tiny_model(kind):
    """6 x 5 mesh, M = 8, C = 16, T = 2, two output frames, B = 3: the summed loss and every parameter after the one step
    against the float64 restatement with torch.optim.AdamW to 2e-5 (the figure of the SequenSolver and LearnSlice training
    tests: one Adam step moves an element by at most lr = 1e-3, and the float32 gradients agree to 1e-5 and better), with
    torch's AdamW and with FusedAdamW; the frozen SequenSolver is left unchanged."""
    from transformerbasednavierstokesolver_amd import harness
    from transformerbasednavierstokesolver_amd.optim import FusedAdamW
    seq, make, sd, fwd, code_and_target, x, fx, yy = _tiny_setup(kind, 21)
    sd_seq = {k: v.detach().clone() for k, v in seq.state_dict().items()}
    want_loss, want, read = _restated_train_step(sd_seq, sd, fwd, code_and_target, x, fx, yy, torch.float64)
    seq = seq.cuda().eval()
    for p in seq.parameters():
        p.requires_grad = False
    results = {}
    for opt_kind in ("torch", "fused"):
        m = _load(make(), sd).train()
        if opt_kind == "torch":
            opt, sync = torch.optim.AdamW(m.parameters(), **HYPER), None
        else:
            opt = FusedAdamW(m.parameters(), **HYPER)
            sync = opt.sync
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda step: 1.0)
        loss = harness.slice_predictor_train_step(m, opt, sched, seq, x.cuda(), fx.cuda(), yy.cuda(), grad_sync=sync)
        assert sched.last_epoch == 1                                    # one optimizer step per batch
        print(f"slice_predictor_train_step {kind} {opt_kind}: loss {float(loss):.9g} against {want_loss:.9g}")
        np.testing.assert_allclose(float(loss), want_loss, rtol=2e-5)
        got = {k: v.detach().clone() for k, v in m.state_dict().items()}
        for k in sd:
            err = R.rel(got[k], want[k])
            print(f"  {opt_kind} {k}: rel-L2 {err:.3g}")
            assert err <= 2e-5, (opt_kind, k, err)
            if read[k]:
                assert not torch.equal(got[k].cpu(), torch.from_numpy(sd[k])), k       # every parameter the forward reads moved
        results[opt_kind] = (float(loss), got)
    np.testing.assert_allclose(results["fused"][0], results["torch"][0], rtol=2e-5)
    for k in sd:
        assert R.rel(results["fused"][1][k], results["torch"][1][k]) <= 2e-5, k
    for k, v in seq.state_dict().items():
        assert torch.equal(v.cpu(), sd_seq[k]), k


@pytest.mark.parametrize("kind", ["vorticity", "slicelearner"])
def test_slice_predictor_rollout_on_a_tiny_model(kind):
    """Three steps with the prediction fed back, against the restated loop (LearnSlice.py:861-913) in float64; the yardstick
    is the same loop in float32 on the CPU."""
    import sequensolver_restatement as S
    from oracle import transolver_oracle as orc
    from transformerbasednavierstokesolver_amd import harness
    seq, make, sd, fwd, code_and_target, x, fx, _ = _tiny_setup(kind, 31)
    sd_seq = {k: v.detach().clone() for k, v in seq.state_dict().items()}

    def restated(dtype):
        s = {k: v.to(dtype) for k, v in sd_seq.items()}
        own = S.split_state_dict(s)[1]
        P = R.to_torch(sd, dtype)
        xx, w = x.to(dtype), fx.to(dtype)
        preds = []
        with torch.no_grad():
            for _ in range(3):
                code, _ = code_and_target(s, xx, w, None)
                decoded = orc.deslice(fwd(P, xx, w, code), code)
                pred = orc.layer_norm(decoded, own["ln_3.weight"], own["ln_3.bias"]) @ own["mlp2.weight"].t() + own["mlp2.bias"]
                preds.append(pred)
                w = torch.cat((w[..., 1:], pred), dim=-1)
        return torch.cat(preds, -1)

    r64, r32 = restated(torch.float64), restated(torch.float32)
    seq = seq.cuda().eval()
    m = _load(make(), sd).eval()
    before = fx.clone()
    got = harness.slice_predictor_rollout(m, seq, x.cuda(), fx.cuda(), 3)
    assert got.shape == (3, 30, 3) and torch.equal(fx, before)
    _bounded("pred", got.reshape(3, -1), r64.reshape(3, -1), r32.reshape(3, -1), f"slice_predictor_rollout {kind} 3 steps")
    assert not torch.equal(got[..., 0], got[..., 1])                     # the prediction entered the window
