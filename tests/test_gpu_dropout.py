"""Training-mode dropout on the MI355X: the flat output kernel against the host mask, token attention with a
dropped attention matrix against the fp64 restatement (tests/dropout_restatement.py), and the served models against the
reference-made fixture tests/golden/G24_dropout.npz and the restatement.

Bounds.  dropout_residual: dropped elements are `res` exactly; kept ones |got - ref64| <= 2^-22 (|res| + |z| / (1 - p)): one
rounding (2^-24 relative) each of the scale, of the product and of the sum, the latter two on magnitudes bounded by the
two terms.  Token attention: per-row rel-L2 against fp64 within elementwise_check.ROW_TOL["f32"] (the token kernels are
exact fp32 on every engine), the bound tests/test_gpu_elementwise.py applies to o, ds and dn of the present kernels; the
weight gradients are checked per row of [D, D] with the same bound.  Models: the tolerances of tests/test_gpu_model.py for
G1 / G6 (forward 1e-5, gradients 1e-4, to_q / to_k 2e-3).  Worst values of a run are printed at the end (pytest -s).

Measured on the MI355X: dropout_residual 0.69 of its bound (n = 3 trips + 3, p = 0.1, with res); token attention worst row
rel-L2 o 8.6e-7, ds 9.2e-7, dn 8.9e-7, dwq 1.1e-6, dwk 1.2e-6, dwv 1.2e-6 (bound 1.9e-5: ROW_TOL carries over); models forward
2.8e-7 .. 3.8e-7, gradients at most 0.044 of their tolerance on the f32 and split engines.  bf16 engine (bound: 4 x its own
dropout-free error, see BF16_SLACK): forward 1.04e-2 with dropout against 1.38e-2 without; gradients 5.5e-3 .. 6.7e-2 with
against 5.7e-3 .. 8.4e-2 without, the largest ratio with / without 1.76 (blocks.1.Attn.temperature, 6.70e-2 / 3.80e-2)."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_l2
from elementwise_check import ROW_TOL, check_rows, poisoned
import dropout_restatement as dr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G24 = os.path.join(GOLDEN, "G24_dropout.npz")
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst values (dropout):")
    for k in sorted(WORST):
        print(f"  {k:40s} {WORST[k][0]:.3e}   {WORST[k][1]}")


def _note(key, v, label):
    if key not in WORST or v > WORST[key][0]:
        WORST[key] = (v, label)


def _grad_tol(key):
    return 2e-3 if ("to_q" in key or "to_k" in key) else 1e-4


# The one-term bf16 engine (fp32 storage), a case this file adds beyond the fp32-accurate ones the models are specified on.
# Its products round both operands to 8 bits, and what that does to a gradient depends on the model (sharp softmaxes from
# clamped temperatures, as in this case's weights), not on dropout: the suite has no calibrated bound for this shape.  So
# the yardstick is the engine's OWN error: the same model, weights, inputs and engine with dropout = 0 against the fp64
# restatement without masks.  With dropout every output and gradient has to come within BF16_SLACK times that error, or
# times one bf16 rounding (2^-8) where the dropout-free error happens to be smaller: dropout removes terms and scales the
# kept ones by 1 / (1 - p), which leaves each product's relative rounding as it was and changes only how much the terms
# cancel; 4 is this suite's factor between a measured error and its bound.
BF16_SLACK, BF16_UNIT = 4.0, 2.0 ** -8


# ---------------------------------------------------------------------------------------------- dropout_residual
def _host_keep(seed, offset, n, thresh):
    from transformerbasednavierstokesolver_amd import ops
    return ops.dropout_keep_host(seed, offset, 0, n, thresh).to(DEV).bool()


def _sizes():
    from transformerbasednavierstokesolver_amd import ops
    return [1, 4 * 37 + 3, 3 * ops.DROPOUT_TRIP + 3]


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("shift,offset", [(0, 0), (1, 11), (0, 2 ** 32 - 3)])
def test_dropout_residual_ones_equal_host_mask(which, shift, offset):
    """z = 1, res = None: keep * scale bit for bit, on the 16-byte path, on a view one element off it (4-byte aligned
    only), and with counters that cross 2^32."""
    from transformerbasednavierstokesolver_amd import ops
    n = _sizes()[which]
    if which == 2 and offset == 2 ** 32 - 3:
        n = 4 * 37 + 2              # the carry is three groups in: the large size adds nothing to it
    p, seed = 0.25, 0xC0FFEE1234567
    thresh, scale = ops.dropout_constants(p)
    z = torch.ones(n + shift, dtype=torch.float32, device=DEV)[shift:]
    assert z.data_ptr() % 16 == 4 * shift and z.is_contiguous()
    out = poisoned(ops.dropout_residual, z, None, (thresh, scale, seed, offset))
    keep = _host_keep(seed, offset, n, thresh)
    want = torch.where(keep, torch.full_like(out, scale), torch.zeros_like(out))
    assert torch.equal(out, want), f"{int((out != want).sum())} of {n} elements differ; first at {int((out != want).nonzero()[0])}"
    assert not torch.signbit(out).any()


@pytest.mark.parametrize("which", [1, 2])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("with_res", [True, False])
def test_dropout_residual_values(which, p, with_res):
    from transformerbasednavierstokesolver_amd import ops
    n = _sizes()[which]
    g = torch.Generator(device=DEV).manual_seed(n % 1000 + int(100 * p))
    z = torch.randn(n, device=DEV, generator=g)
    res = torch.randn(n, device=DEV, generator=g) if with_res else None
    thresh, scale = ops.dropout_constants(p)
    seed, offset = 991, 5
    out = poisoned(ops.dropout_residual, z, res, (thresh, scale, seed, offset))
    keep = _host_keep(seed, offset, n, thresh)
    base = res if with_res else torch.zeros_like(z)
    assert torch.equal(out[~keep], base[~keep])                       # dropped: res exactly (+0.0 without one)
    if not with_res:
        assert not torch.signbit(out[~keep]).any()
    term = z.double().abs() / (1.0 - p)
    ref = base.double() + z.double() / (1.0 - p)
    err = (out.double() - ref).abs()[keep]
    bound = (2.0 ** -22 * (base.double().abs() + term))[keep]
    ratio = float((err / bound.clamp_min(1e-300)).max())
    _note("dropout_residual |err| / bound", ratio, f"n={n} p={p} res={with_res}")
    assert ratio <= 1.0, ratio
    if n > 10 ** 6:                  # sigma <= 2e-4 at this size
        assert abs(float(keep.double().mean()) - (1 - p)) < 2e-3


# ---------------------------------------------------------------------------------------------- token attention
def _token_inputs(case):
    return {k: torch.from_numpy(v).to(DEV) for k, v in dr.token_case(*case, seed=sum(case)).items()}


def _token_run(t, drop):
    from transformerbasednavierstokesolver_amd import ops
    s, nrm, o = poisoned(ops.token_attn_fwd, t["spart"], t["npart"], t["wq"], t["wk"], t["wv"], drop=drop)
    ds, dn, dwq, dwk, dwv = poisoned(ops.token_attn_bwd, s, nrm, t["wq"], t["wk"], t["wv"], t["dopart"], drop=drop)
    return dict(o=o, ds=ds, dn=dn, dwq=dwq, dwk=dwk, dwv=dwv)


@pytest.mark.parametrize("p", dr.TOKEN_PS)
@pytest.mark.parametrize("case", dr.TOKEN_CASES)
def test_token_attention_dropout_against_fp64(case, p):
    from transformerbasednavierstokesolver_amd import ops
    BH, M, D, nchunk = case
    thresh, scale = ops.dropout_constants(p)
    seed = dr.token_seed(*case, p)
    mask, rows = dr.token_mask(*case, p)
    host = ops.dropout_keep_host(seed, dr.TOKEN_OFFSET, 0, BH * M * M, thresh).numpy().reshape(BH, M, M)
    assert np.array_equal(host, mask)
    assert (~rows).sum() * 8 <= rows.size
    got = _token_run(_token_inputs(case), (thresh, scale, seed, dr.TOKEN_OFFSET))
    ref = dr.token_reference(dr.token_case(*case, seed=sum(case)), mask, scale)
    tag = f"token dropout BH={BH} M={M} D={D} nchunk={nchunk} p={p}"
    live = torch.from_numpy(rows.reshape(-1))
    o = got["o"].cpu().reshape(-1, D)
    assert not o[~live].any(), "rows whose mask keeps nothing have to be exact zeros in o"
    tol = ROW_TOL["f32"]
    for key, g, r in (("o", o[live], ref["o"].reshape(-1, D)[live]), ("ds", got["ds"].reshape(-1, D), ref["ds"].reshape(-1, D)),
                      ("dn", got["dn"].reshape(BH, M), ref["dn"].reshape(BH, M)), ("dwq", got["dwq"], ref["dwq"]),
                      ("dwk", got["dwk"], ref["dwk"]), ("dwv", got["dwv"], ref["dwv"])):
        rel = (g.double().cpu() - r).norm(dim=1) / r.norm(dim=1).clamp_min(1e-300)
        print(f"{tag} {key}: worst row rel-L2 {float(rel.max()):.3e}")
        _note(f"token {key} row rel-L2", float(rel.max()), tag)
    for key, g, r in (("o", o[live], ref["o"].reshape(-1, D)[live]), ("ds", got["ds"].reshape(-1, D), ref["ds"].reshape(-1, D)),
                      ("dn", got["dn"].reshape(BH, M), ref["dn"].reshape(BH, M)), ("dwq", got["dwq"], ref["dwq"]),
                      ("dwk", got["dwk"], ref["dwk"]), ("dwv", got["dwv"], ref["dwv"])):
        check_rows(g.cpu(), r, tol, label=f"{tag} {key}")


@pytest.mark.parametrize("case", dr.TOKEN_CASES)
def test_token_attention_dropout_edges(case):
    from transformerbasednavierstokesolver_amd import ops
    BH, M, D, nchunk = case
    t = _token_inputs(case)
    plain = _token_run(t, None)
    keep_all = _token_run(t, (0, 1.0, 31337, 2 ** 40 + 3))
    for k in plain:                       # thresh 0, scale 1: the present entry points, bit for bit
        assert torch.equal(plain[k], keep_all[k]), k
    seed, offset = 4242, 17
    assert not ops.dropout_keep_host(seed, offset, 0, BH * M * M, 2 ** 32 - 1).any()
    none = _token_run(t, (2 ** 32 - 1, 2.0, seed, offset))
    for k, v in none.items():             # nothing kept: exact zeros (either sign), forward and every gradient
        assert not v.any(), k


# ---------------------------------------------------------------------------------------------- models
def _g24(tag):
    g = np.load(G24)
    pre = tag + "."
    cfg = json.loads(str(g[pre + "config"]))
    sd = {k[len(pre) + 3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre + "sd.")}
    return g, pre, cfg, sd


def _build(kind, cfg, sd, engine, dropout, geom=None):
    from transformerbasednavierstokesolver_amd.model import (Transolver_Irregular_Mesh, Transolver_Structured_Mesh_2D,
                                                             Transolver_Structured_Mesh_3D)
    kw = dict(n_layers=cfg["n_layers"], n_hidden=cfg["n_hidden"], dropout=dropout, n_head=cfg["n_head"], Time_Input=False,
              mlp_ratio=cfg["mlp_ratio"], fun_dim=cfg["fun_dim"], out_dim=cfg["out_dim"], slice_num=cfg["slice_num"],
              ref=cfg.get("ref", 8), unified_pos=cfg.get("unified_pos", 0))
    if kind == "2d":
        m = Transolver_Structured_Mesh_2D.Model(space_dim=2, H=cfg["H"], W=cfg["W"], **kw)
    elif kind == "3d":
        m = Transolver_Structured_Mesh_3D.Model(space_dim=3, H=geom[0], W=geom[1], D=geom[2], **kw)
    else:
        m = Transolver_Irregular_Mesh.Model(space_dim=2, **kw)
    if sd is not None:
        res = m.load_state_dict(sd, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
    return m.to(DEV).set_engine(engine)


@pytest.mark.parametrize("engine", ["f32", "split"])
@pytest.mark.parametrize("tag", ["2d", "irregular"])
def test_g24_reference_made_fixture(tag, engine):
    from transformerbasednavierstokesolver_amd import ops
    g, pre, cfg, sd = _g24(tag)
    m = _build(tag, cfg, sd, engine, float(g[pre + "p"])).train()
    x, fx, gy = (torch.from_numpy(g[pre + k]).to(DEV) for k in ("x", "fx", "gy"))
    ops.dropout_manual_seed(int(g[pre + "seed"]))
    pred = m(x, fx)
    pred.backward(gy)
    B, N = x.shape[:2]
    per_layer = (B * cfg["n_head"] * cfg["slice_num"] ** 2 + 3) // 4 + (B * N * cfg["n_hidden"] + 3) // 4
    assert ops.dropout_state() == (int(g[pre + "seed"]), cfg["n_layers"] * per_layer)
    e = rel_l2(pred, g[pre + "pred.f64"])
    _note(f"G24 {tag} forward rel-L2", e, engine)
    assert e < 1e-5, e
    for k, p in m.named_parameters():
        if pre + "grad.f64." + k not in g.files:
            assert p.grad is None or not p.grad.any(), k
            continue
        e = rel_l2(p.grad, g[pre + "grad.f64." + k])
        _note(f"G24 {tag} grad rel-L2 / tol", e / _grad_tol(k), f"{engine} {k}")
        assert e < _grad_tol(k), (k, e)


def _restated_case(kind, engine):
    """A model of `kind` with seeded weights, its inputs, and the fp64 restatement's output and gradients for the draws the
    package makes from (seed 606, offset 0)."""
    from transformerbasednavierstokesolver_amd import ops, synth
    p = 0.25
    if kind == "3d":             # G8's tiny shape
        geom, B = (4, 5, 3), 2
        cfg = dict(n_layers=2, n_hidden=32, n_head=4, mlp_ratio=2, fun_dim=1, out_dim=2, slice_num=8, unified_pos=0)
        sdim = 3
    else:                        # 2-D, served by the operand-planes route on the split engine
        geom, B = (9, 7), 2
        cfg = dict(n_layers=2, n_hidden=128, n_head=8, mlp_ratio=1, fun_dim=3, out_dim=1, slice_num=12, unified_pos=0,
                   H=9, W=7)
        sdim = 2
        assert ops.conv_planes_mask(B, 9, 7, 128, "split") == 7
    m = _build(kind, cfg, None, engine, p, geom)
    spec = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict_from_spec(spec, seed=61, wild_temperature=True).items()}
    m.load_state_dict(sd, strict=True)
    N = int(np.prod(geom))
    rng = np.random.default_rng(62)
    x = torch.from_numpy(rng.uniform(0, 1, (B, N, sdim)).astype(np.float32))
    fx = torch.from_numpy(rng.standard_normal((B, N, cfg["fun_dim"])).astype(np.float32))
    gy = torch.from_numpy(rng.standard_normal((B, N, cfg["out_dim"])).astype(np.float32))
    thresh, scale = ops.dropout_constants(p)
    masks, _ = dr.layer_masks(606, 0, thresh, cfg["n_layers"], B, cfg["n_head"], cfg["slice_num"], N, cfg["n_hidden"])
    sdo = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    ref = dr.model_forward(sdo, x.double(), fx.double(), kind, geom, cfg, masks, scale)
    ref.backward(gy.double())
    return m, x, fx, gy, ref.detach(), {k: v.grad for k, v in sdo.items()}, (kind, cfg, geom, sd)


def _engine_error_without_dropout(case, engine, x, fx, gy):
    """rel-L2 of the dropout-free model (same weights, same engine, training mode) against the fp64 restatement with all-ones
    masks: (forward, {parameter: gradient}).  The yardstick of the bf16-engine case."""
    kind, cfg, geom, sd = case
    m0 = _build(kind, cfg, sd, engine, 0.0, geom).train()
    pred = m0(x.to(DEV), fx.to(DEV))
    pred.backward(gy.to(DEV))
    B, N = x.shape[:2]
    ones = [(torch.ones(B, cfg["n_head"], cfg["slice_num"], cfg["slice_num"], dtype=torch.float64),
             torch.ones(B, N, cfg["n_hidden"], dtype=torch.float64)) for _ in range(cfg["n_layers"])]
    sdo = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    ref = dr.model_forward(sdo, x.double(), fx.double(), kind, geom, cfg, ones, 1.0)
    ref.backward(gy.double())
    return rel_l2(pred, ref.detach()), {k: rel_l2(p.grad, sdo[k].grad) for k, p in m0.named_parameters()
                                        if sdo[k].grad is not None}


@pytest.mark.parametrize("kind,engine", [("3d", "f32"), ("3d", "split"), ("2d", "split"), ("2d", "bf16")])
def test_3d_and_planes_route_against_restatement(kind, engine):
    from transformerbasednavierstokesolver_amd import ops
    m, x, fx, gy, ref, grads, case = _restated_case(kind, engine)
    bf = engine == "bf16"
    e0_fwd, e0 = _engine_error_without_dropout(case, engine, x, fx, gy) if bf else (None, None)
    ops.dropout_manual_seed(606)
    pred = m.train()(x.to(DEV), fx.to(DEV))
    pred.backward(gy.to(DEV))
    e = rel_l2(pred, ref)
    _note(f"restated {kind} forward rel-L2", e, engine)
    if bf:
        print(f"bf16 engine forward: without dropout {e0_fwd:.3e}, with {e:.3e}")
    assert e < (BF16_SLACK * max(e0_fwd, BF16_UNIT) if bf else 1e-5), e
    bad = []
    for k, p in m.named_parameters():
        if grads[k] is None:
            assert p.grad is None or not p.grad.any(), k
            continue
        e = rel_l2(p.grad, grads[k])
        tol = BF16_SLACK * max(e0[k], BF16_UNIT) if bf else _grad_tol(k)
        if bf:
            print(f"bf16 engine {k}: without dropout {e0[k]:.3e}, with {e:.3e}")
        _note(f"restated {kind} grad rel-L2 / tol", e / tol, f"{engine} {k}")
        if not e < tol:
            bad.append((k, e, tol))
    assert not bad, bad


def _tiny(dropout, seed=3):
    torch.manual_seed(seed)
    cfg = dict(n_layers=2, n_hidden=32, n_head=4, mlp_ratio=2, fun_dim=3, out_dim=1, slice_num=8, unified_pos=0, H=6, W=5)
    return _build("2d", cfg, None, "split", dropout)


def _tiny_inputs(B=2, T=1):
    g = torch.Generator().manual_seed(9)
    return (torch.rand(B, 30, 2, generator=g).to(DEV), torch.randn(B, 30, 3, generator=g).to(DEV),
            torch.randn(B, 30, T, generator=g).to(DEV))


def test_eval_ignores_dropout_and_leaves_the_generator_alone():
    from transformerbasednavierstokesolver_amd import ops
    x, fx, _ = _tiny_inputs()
    a, b = _tiny(0.25).eval(), _tiny(0.0).eval()
    ops.dropout_manual_seed(12)
    ops.dropout_reserve(40)
    state = ops.dropout_state()
    with torch.no_grad():
        ya, yb = a(x, fx), b(x, fx)
    assert torch.equal(ya, yb) and ops.dropout_state() == state == (12, 10)
    # ... with gradients recorded too, and a p = 0 model in training mode draws nothing either
    ya, yb = a(x, fx), b.train()(x, fx)
    assert torch.equal(ya, yb) and ops.dropout_state() == state


def test_training_calls_differ_and_reseeding_reproduces():
    from transformerbasednavierstokesolver_amd import ops
    x, fx, _ = _tiny_inputs()
    m = _tiny(0.25).train()
    ops.dropout_manual_seed(99)
    y1 = m(x, fx).detach().clone()
    y2 = m(x, fx).detach().clone()
    assert not torch.equal(y1, y2) and torch.isfinite(y1).all() and torch.isfinite(y2).all()
    ops.dropout_manual_seed(99)
    assert torch.equal(m(x, fx).detach(), y1)
    torch.manual_seed(1234)                # without an explicit seed the generator follows torch's
    y3 = m(x, fx).detach().clone()
    assert ops.dropout_state()[0] == 1234
    torch.manual_seed(1235)
    assert ops.dropout_state() == (1235, 0)
    torch.manual_seed(1234)
    assert torch.equal(m(x, fx).detach(), y3)


def test_fused_tail_flag_does_not_skip_dropout():
    from transformerbasednavierstokesolver_amd import ops
    x, fx, _ = _tiny_inputs()
    m = _tiny(0.25).train()
    with torch.no_grad():
        ops.dropout_manual_seed(7)
        off = m(x, fx).clone()
        m.set_fused_tail(True)
        ops.dropout_manual_seed(7)
        on = m(x, fx).clone()
        assert ops.dropout_state()[1] > 0
    assert torch.equal(on, off)


def test_two_train_steps_with_dropout():
    from transformerbasednavierstokesolver_amd import harness, ops
    x, fx, yy = _tiny_inputs(T=2)

    def run():
        m = _tiny(0.1).train()
        before = [p.detach().clone() for p in m.parameters()]
        opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-5)
        ops.dropout_manual_seed(5)
        losses = [harness.train_step(m, opt, None, x, fx, yy)[0] for _ in range(2)]
        assert all(torch.isfinite(v) for v in losses)
        assert any(not torch.equal(a, p.detach()) for a, p in zip(before, m.parameters()))
        return m, losses

    (m1, l1), (m2, l2) = run(), run()
    assert all(torch.equal(a, b) for a, b in zip(l1, l2))
    for (k, p), q in zip(m1.named_parameters(), m2.parameters()):
        assert torch.equal(p, q), k
