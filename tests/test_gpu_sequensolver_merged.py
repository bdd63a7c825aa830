"""The merged SequenSolver on the MI355X: the fused head attention (pa2d_head_seq_attn_*) and the causal mode of
pa2d_seq_attn_* element by element against a torch float64 restatement (tests/sequensolver_merged_restatement.py), the two
routes of functional.head_seq_attention against each other, and the whole model against the reference's results in
tests/golden/G13_sequensolver_merged.npz (written by tools/make_golden_sequensolver_merged.py).

Per-row bounds of the stages, as in test_gpu_sequensolver.py: the yardstick is the same restatement evaluated by torch in
float32 on the CPU against its float64 result on the test's own inputs, and the bound is 4 x its worst row error.  Every
test prints the measured GPU value beside the bound before it asserts.  The model is held to the project's acceptance
bounds exactly as test_gpu_sequensolver.py derives them (forward 1e-5, gradients 1e-4, to_q / to_k 2e-3, losses 2e-5, or
4 x the fixture's recorded fp32 self error where that exceeds a quarter of the bound).

Shapes (G, T, sd) of the stage tests, small on purpose: (1, 1, 4) the smallest; (3, 3, 12) odd sizes; (16, 10, 32) the
reference's; (5, 32, 64) both maxima (more than 64 KiB of LDS: the raised limit); (40, 7, 20) more groups than workgroups
(32), so that workgroups walk several groups and the fixed-order record sum runs over the full record count."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_l2
from elementwise_check import check_rows, poisoned
import sequensolver_merged_restatement as R
from test_gpu_sequensolver import _acceptance, _bound, _bounded, _close, _loss, _row_err, _rows, _zero
from test_sequensolver_merged_host import TINY_ENCODER

pytestmark = pytest.mark.gpu

HEAD_SHAPES = [(1, 1, 4), (3, 3, 12), (16, 10, 32), (5, 32, 64), (40, 7, 20)]
HEAD_CASES = [(G, T, sd, causal, with_res, 1.0) for G, T, sd in HEAD_SHAPES for causal in (0, 1) for with_res in (True, False)]
HEAD_CASES.append((16, 10, 32, 1, True, 30.0))      # q times 30: logits spread so wide that the softmax is near one-hot
NAMES = ("out", "dx", "dwq", "dwk", "dwv")


def _head_operands(G, T, sd, spread, seed):
    g = torch.Generator().manual_seed(seed)
    x, res, dout = (torch.randn(G, T, sd, generator=g) for _ in range(3))
    wq, wk, wv = (torch.randn(sd, sd, generator=g) / sd ** 0.5 for _ in range(3))
    return x, wq * spread, wk, wv, res, dout


def _head_restated(cpu, dtype, scale, causal, with_res):
    """Every group is one sample with one head of the restatement: (out, dx, dwq, dwk, dwv)."""
    x, wq, wk, wv = (t.to(dtype).clone().requires_grad_(True) for t in cpu[:4])
    res, dout = cpu[4].to(dtype), cpu[5].to(dtype)
    out = R.head_attention(x, wq, wk, wv, 1, scale, causal=bool(causal), res=res if with_res else None)
    out.backward(dout)
    return out.detach(), x.grad, wq.grad, wk.grad, wv.grad


def _head_case(G, T, sd, causal, with_res, spread):
    cpu = _head_operands(G, T, sd, spread, seed=3000 + 101 * G + 7 * T + sd)
    scale = sd ** -0.5
    ref64 = _head_restated(cpu, torch.float64, scale, causal, with_res)
    ref32 = _head_restated(cpu, torch.float32, scale, causal, with_res)
    return cpu, scale, ref64, ref32


@pytest.mark.parametrize("G,T,sd,causal,with_res,spread", HEAD_CASES)
def test_fused_head_attention_forward_backward_rows(G, T, sd, causal, with_res, spread):
    from transformerbasednavierstokesolver_amd import ops
    cpu, scale, ref64, ref32 = _head_case(G, T, sd, causal, with_res, spread)
    x, wq, wk, wv, res, dout = (t.cuda() for t in cpu)
    r = res if with_res else None
    label = f"head_seq_attn G={G} T={T} sd={sd} causal={causal} res={with_res} spread={spread}"
    out, attn = poisoned(ops.head_seq_attn_fwd, x, wq, wk, wv, scale, r, causal)       # twice, equal bits
    assert attn.shape == (G, T, T) and float((attn.sum(-1) - 1).abs().max()) < 1e-5
    if causal:
        assert bool((attn.triu(1) == 0).all()), "attn[i, j > i] must be exactly 0"
    else:
        assert bool((attn > 0).all())
    if spread > 1:
        assert float(attn.max(-1).values.median()) > 0.9, "the spread case is meant to be near one-hot"
    grads = poisoned(ops.head_seq_attn_bwd, x, wq, wk, wv, attn, dout, scale, causal)
    for name, got, r64, r32 in zip(NAMES, (out,) + tuple(grads), ref64, ref32):
        _bounded(name, got, r64, r32, label)
    # accumulate = 1 adds onto a prefilled gradient: one float add per element
    g = torch.Generator().manual_seed(5)
    pre = tuple(torch.randn(sd, sd, generator=g).cuda() for _ in range(3))
    into = tuple(p.clone() for p in pre)
    dx2, *acc = ops.head_seq_attn_bwd(x, wq, wk, wv, attn, dout, scale, causal, into=into)
    assert torch.equal(dx2, grads[0]) and all(a is b for a, b in zip(acc, into))
    assert all(torch.equal(a, p + gr) for a, p, gr in zip(into, pre, grads[1:]))


@pytest.mark.parametrize("G,T,sd,causal,with_res,spread", HEAD_CASES)
def test_unfused_route_and_agreement_of_the_two_routes(G, T, sd, causal, with_res, spread):
    """functional.head_seq_attention on xn [B, T, dim] with heads = G / B groups per sample: fused=False (three linears and
    the causal pa2d_seq_attn) and fused=True against the restatement, and against each other within the same bounds."""
    from transformerbasednavierstokesolver_amd import functional as Fn
    cpu, scale, ref64, ref32 = _head_case(G, T, sd, causal, with_res, spread)
    B = 2 if G % 2 == 0 else 1
    heads = G // B
    label = f"head_seq_attention B={B} heads={heads} T={T} sd={sd} causal={causal} res={with_res} spread={spread}"
    got = {}
    for fused in (False, True):
        xn = cpu[0].reshape(B, T, heads * sd).cuda().requires_grad_(True)      # the [G, T, sd] view of this memory is x
        W = [w.cuda().requires_grad_(True) for w in cpu[1:4]]
        res = cpu[4].reshape(B, T, heads * sd).cuda() if with_res else None
        out = Fn.head_seq_attention(xn, *W, heads, scale, res=res, causal=bool(causal), fused=fused)
        assert out.shape == (B, T, heads * sd)
        out.backward(cpu[5].reshape(B, T, heads * sd).cuda())
        got[fused] = (out.detach().reshape(G, T, sd), xn.grad.reshape(G, T, sd)) + tuple(w.grad for w in W)
        for name, t, r64, r32 in zip(NAMES, got[fused], ref64, ref32):
            _bounded(name, t, r64, r32, f"{label} fused={fused}")
    for name, a, b, r64, r32 in zip(NAMES, got[True], got[False], ref64, ref32):
        tol = 4.0 * _row_err(r32, r64)
        print(f"{label} {name}: fused against unfused, worst row rel-L2 {_row_err(a, b):.3g}, bound {tol:.3g}")
        check_rows(_rows(a), _rows(b), tol, label=f"{label} {name} fused vs unfused")


CAUSAL_STAGE_CASES = [(1, 1, 4, 1.0), (3, 3, 12, 1.0), (5, 10, 128, 1.0), (2, 32, 512, 1.0), (2, 10, 128, 30.0)]


@pytest.mark.parametrize("B,T,dim,spread", CAUSAL_STAGE_CASES)
def test_causal_sequence_attention_stage_rows(B, T, dim, spread):
    from transformerbasednavierstokesolver_amd import ops
    g = torch.Generator().manual_seed(4000 + 7 * T + dim + B)
    q = torch.randn(B, T, dim, generator=g) * spread
    k, v, res, dout = (torch.randn(B, T, dim, generator=g) for _ in range(4))
    scale = dim ** -0.5

    def restated(dtype):
        qq, kk, vv = (t.to(dtype).clone().requires_grad_(True) for t in (q, k, v))
        dots = (qq @ kk.transpose(-1, -2) * scale).masked_fill(torch.tril(torch.ones(T, T)) == 0, float("-inf"))
        out = torch.softmax(dots, -1) @ vv + res.to(dtype)
        out.backward(dout.to(dtype))
        return out.detach(), qq.grad, kk.grad, vv.grad

    ref64, ref32 = restated(torch.float64), restated(torch.float32)
    dev = [t.cuda() for t in (q, k, v, res, dout)]
    out, attn = poisoned(ops.seq_attn_causal_fwd, dev[0], dev[1], dev[2], scale, dev[3])
    assert bool((attn.triu(1) == 0).all()) and float((attn.sum(-1) - 1).abs().max()) < 1e-5
    dq, dk, dv = poisoned(ops.seq_attn_causal_bwd, dev[0], dev[1], dev[2], attn, dev[4], scale)
    label = f"seq_attn causal B={B} T={T} dim={dim} spread={spread}"
    for name, got, r64, r32 in zip(("out", "dq", "dk", "dv"), (out, dq, dk, dv), ref64, ref32):
        _bounded(name, got, r64, r32, label)
    # causal=False of the same wrappers is the plain stage: the last row sees every token, so only it can agree
    plain, _ = ops.seq_attn_fwd(dev[0], dev[1], dev[2], scale, dev[3])
    assert rel_l2(plain[:, -1], out[:, -1]) < 1e-5 and (T == 1 or not torch.equal(plain, out))


def test_refusals_and_empty_batch():
    from transformerbasednavierstokesolver_amd import functional as Fn, ops
    x, w = torch.randn(2, 33, 32, device="cuda"), torch.randn(32, 32, device="cuda")
    with pytest.raises(RuntimeError, match="PA2D_ERR_UNSUPPORTED"):
        ops.head_seq_attn_fwd(x, w, w, w, 1.0)
    x, w = torch.randn(2, 4, 68, device="cuda"), torch.randn(68, 68, device="cuda")
    with pytest.raises(RuntimeError, match="PA2D_ERR_UNSUPPORTED"):
        ops.head_seq_attn_fwd(x, w, w, w, 1.0)
    with pytest.raises(RuntimeError, match="PA2D_ERR_UNSUPPORTED"):
        Fn.head_seq_attention(x, w, w, w, 1, 1.0, fused=True)          # forced: no quiet change of route
    assert Fn.head_seq_attention(x, w, w, w, 1, 1.0).shape == (2, 4, 68)      # seq_dim 68 > 64: the unfused route
    e, w = torch.empty(0, 4, 32, device="cuda"), torch.randn(32, 32, device="cuda")
    out, attn = ops.head_seq_attn_fwd(e, w, w, w, 1.0)
    assert out.shape == (0, 4, 32) and attn.shape == (0, 4, 4)
    dx, *g = ops.head_seq_attn_bwd(e, w, w, w, attn, e, 1.0)
    assert dx.shape == (0, 4, 32) and all(float(t.abs().sum()) == 0.0 for t in g)
    ones = tuple(torch.ones_like(t) for t in g)
    ops.head_seq_attn_bwd(e, w, w, w, attn, e, 1.0, into=ones)
    assert all(bool((t == 1).all()) for t in ones)


# ---------------------------------------------------------------------------------------------- the model against G13
G13 = os.path.join(GOLDEN, "G13_sequensolver_merged.npz")
ENGINES = [None, "f32"]          # the default engine (the fp32-accurate split) and exact fp32


@pytest.fixture(scope="module")
def g13():
    return np.load(G13)


def _golden_model(g13, case, engine):
    from transformerbasednavierstokesolver_amd.SequenSolverMerged import SequenSolver
    cfg, geom = json.loads(str(g13[case + ".config"])), json.loads(str(g13["geometry"]))
    sd = {k: torch.from_numpy(v) for k, v in R.golden_state_dict(g13, case).items()}
    enc = {k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}
    m = SequenSolver(enc, T=cfg["T"], layers=cfg["layers"], B=cfg["B"], sequential_head=cfg["sequential_head"], **geom)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().set_engine(engine)
    return m, tuple(torch.from_numpy(a).cuda() for a in R.golden_inputs(g13, case))


def _check_grads(g13, pre, m, label):
    none = []
    for k, p in m.named_parameters():
        if p.grad is None:
            none.append(k)
        else:
            _close(g13, pre + "grad." + k, p.grad, label)
    assert none == json.loads(str(g13[pre + "no_grad"])), label


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("case", ["a", "b"])
def test_model_matches_reference(g13, case, engine):
    m, (pos, fx, y, _) = _golden_model(g13, case, engine)
    label = f"G13 {case} engine={engine}"
    assert (m.seq_dim <= 64) == (case == "b")          # case a runs the unfused route, case b the fused kernel
    out = m(pos, fx, y, use_gt=False)
    for key, got in (("out", out), ("code", m.code), ("slice_weights", m.slice_weights)):
        _close(g13, f"{case}.pred.{key}", got, label)
    assert abs(float(m.slice_weights.sum()) - out.shape[0] * m.N) < 1e-5 * out.shape[0] * m.N
    assert float(m.temperature) == 0.5 and m.temperature.is_cuda
    loss = _loss(out, y)
    _close(g13, f"{case}.pred.loss", loss, label)
    loss.backward()
    _check_grads(g13, f"{case}.pred.", m, label)
    with torch.no_grad():
        _close(g13, f"{case}.get_code", m.get_code(pos, fx, y), label)
        if case == "a":      # use_gt=True: the same output, and the encoder's cached slice weights are those of y
            out_gt = m(pos, fx, y, use_gt=True)
            _close(g13, "a.gt.out", out_gt, label)
            assert rel_l2(out_gt, out) <= 1e-5            # the encoder ran a batch of 11 frames instead of 10: not the same bits
            cached = m.encoder.get_attention_slice().clone()
            m.encoder.encode(pos, y)
            assert rel_l2(cached, m.encoder.get_attention_slice()) <= 1e-5
        else:                # the other route of the attention meets the same bounds
            m.fused = False
            _close(g13, "b.pred.out", m(pos, fx, y, use_gt=False), label + " unfused")
            m.fused = None
    _zero(m)
    m.train()
    m.freeze_attention()
    frozen = [k for k, p in m.named_parameters() if not p.requires_grad and not k.startswith("encoder.")]
    assert frozen == json.loads(str(g13[f"{case}.frozen.names"]))
    loss = _loss(m(pos, fx, y, use_gt=False), y)
    _close(g13, f"{case}.frozen.loss", loss, label)
    loss.backward()
    _check_grads(g13, f"{case}.frozen.", m, label)


@pytest.mark.parametrize("engine", ENGINES)
def test_training_loop_and_rollout_match_reference(g13, engine):
    from transformerbasednavierstokesolver_amd import harness
    from transformerbasednavierstokesolver_amd.optim import FusedAdamW
    hyper = json.loads(str(g13["train.hyper"]))
    label = f"G13 a engine={engine}"
    m, (pos, fx, _, yy) = _golden_model(g13, "a", engine)
    m.eval()
    with torch.no_grad():
        pred, step_loss, full_loss = harness.sequensolver_rollout(m, pos, fx, yy, use_gt=False)
    _close(g13, "a.rollout.pred", pred, label)
    _close(g13, "a.rollout.step_loss", step_loss, label)
    _close(g13, "a.rollout.full_loss", full_loss, label)
    opt = FusedAdamW(m.parameters(), lr=hyper["lr"], weight_decay=hyper["weight_decay"])
    assert len(opt.sync.params) == sum(1 for p in m.parameters() if p.requires_grad)      # the frozen encoder stays out
    assert all(p is not m.temperature for p in opt.sync.params)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=hyper["lr"], epochs=hyper["epochs"],
                                                steps_per_epoch=hyper["steps_per_epoch"])
    losses = []
    for _ in range(hyper["steps"]):
        m.train()
        loss, _ = harness.sequensolver_train_step(m, opt, sched, pos, fx, yy, use_gt=False, grad_sync=opt.sync)
        losses.append(float(loss))
    want = g13["a.train.losses"]
    rtol = _bound(g13, "a.train.losses")
    print(f"{label} training losses {losses} against {want.tolist()}, rtol {rtol:.3g}")
    np.testing.assert_allclose(losses, want, rtol=rtol)
    assert float(m.temperature) == 0.5


# ---------------------------------------------------------------------------------------------- a shape off the reference's
def _tiny_restated(sd, dtype, x, fx, y):
    sd = {k: v.to(dtype).clone().requires_grad_(not k.startswith("encoder.")) for k, v in sd.items()}
    out, code, sw = R.forward(sd, TINY_ENCODER, 2, 8, x.to(dtype), fx.to(dtype), y.to(dtype))
    loss = R.rel_l2_loss(out, y.to(dtype))
    loss.backward()
    res = {"out": out.detach(), "code": code.detach(), "slice_weights": sw.detach(), "loss": loss.detach()}
    res.update({"grad." + k: v.grad for k, v in sd.items() if v.grad is not None})
    return res


@pytest.mark.parametrize("engine", ENGINES)
def test_tiny_model_off_the_reference_shape(engine):
    """2-layer encoder, 8 x 8 mesh, M=8, C=16, sequential_head=8 (seq_dim 16), T=3, B=2 through `encoder_config`, against
    the float64 restatement; bounds as for G13, with the float32 CPU restatement in the role of the fixture's self error."""
    from transformerbasednavierstokesolver_amd.SequenSolverMerged import SequenSolver
    torch.manual_seed(7)
    m = SequenSolver(None, T=3, W=8, H=8, M=8, C=16, B=2, sequential_head=8, layers=2, encoder_config=TINY_ENCODER)
    with torch.no_grad():      # spread the predicted slice weights, and give every parameter a non-trivial value
        for k, p in m.named_parameters():
            if k.endswith(".bias") or k.startswith("ln_"):
                p.add_(0.1 * torch.randn_like(p))
        m.in_project_slice.linear_post.weight.mul_(4.0)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(8)
    x = torch.from_numpy(R.unified_positions(8, 8)).repeat(2, 1, 1)
    fx, y = torch.randn(2, 64, 3, generator=g), torch.randn(2, 64, 1, generator=g)
    r64 = _tiny_restated(sd, torch.float64, x, fx, y)
    r32 = _tiny_restated(sd, torch.float32, x, fx, y)
    m = m.cuda().set_engine(engine)
    out = m(x.cuda(), fx.cuda(), y.cuda(), use_gt=False)
    loss = _loss(out, y.cuda())
    loss.backward()
    got = {"out": out, "code": m.code, "slice_weights": m.slice_weights, "loss": loss}
    got.update({"grad." + k: p.grad for k, p in m.named_parameters() if p.grad is not None})
    assert sorted(got) == sorted(r64)
    for k, want in r64.items():
        base, own = _acceptance("." + k), rel_l2(r32[k], want)
        bound = 4 * own if own > base / 4 else base
        err = rel_l2(got[k], want)
        print(f"tiny engine={engine} {k}: rel-L2 {err:.3g}, bound {bound:.3g}")
        assert err <= bound, (k, err, bound)


def test_fused_route_accumulates_into_the_gradient_bucket():
    """With optim.FusedAdamW every trainable parameter's gradient is a view of one flat bucket and the fused attention's
    backward adds into it (accumulate = 1), once per weight-tied layer; without the bucket autograd adds the layers' results.
    Same kernels and values, only the fp32 additions of the two layers' terms may associate differently: 1e-6."""
    from transformerbasednavierstokesolver_amd.SequenSolverMerged import SequenSolver
    from transformerbasednavierstokesolver_amd.optim import FusedAdamW
    torch.manual_seed(11)
    m = SequenSolver(None, T=3, W=8, H=8, M=8, C=16, B=1, sequential_head=8, layers=2, encoder_config=TINY_ENCODER).cuda()
    g = torch.Generator().manual_seed(12)
    x = torch.from_numpy(R.unified_positions(8, 8)).cuda()
    fx, y = torch.randn(1, 64, 3, generator=g).cuda(), torch.randn(1, 64, 1, generator=g).cuda()
    _loss(m(x, fx, y, use_gt=False), y).backward()
    plain = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    assert {"to_q.weight", "to_k.weight", "to_v.weight"} <= set(plain)
    _zero(m)
    opt = FusedAdamW(m.parameters(), lr=1e-3)
    opt.zero_grad()
    _loss(m(x, fx, y, use_gt=False), y).backward()
    opt.sync()
    for k, p in m.named_parameters():
        if k in plain:
            slot = next(i for i, q in enumerate(opt.sync.params) if q is p)
            assert p.grad.data_ptr() == opt.sync.views[slot].data_ptr(), k
            err = rel_l2(p.grad, plain[k])
            assert err <= 1e-6, (k, err)
