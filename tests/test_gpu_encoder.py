"""Structured 2-D auto-encoder family on the MI355X: the four new kernels (pa2d_slice_weights_*, pa2d_deslice_weights_*)
element by element against CPU fp64, the model and the attention module against the reference's fp64 outputs
(tests/golden/G9_encoder.npz, tools/make_golden_encoder.py) on the f32, split and bf16 engines, the stateful
encode / decode / get / set interface, and the training plumbing (flat gradient bucket, FusedAdamW, three
auto_encoder.py iterations).

Per-element bounds (check_products: |got - ref| <= tau * scale).  The kernels are exact fp32 on every engine (VALU FMA).
Scales: de-slice forward |w| |code|; its backward |w|^T |dy| (dcode) and |dy| |code|^T (dw).  Slice weights: the softmax
error bound sw * (1 + L + max_m L) with L = (|x| |Ws|^T + |bs|) / t the logit magnitude; its backward runs on
dz = sw (|dsw| + |<sw, dsw>|) (1 + max_m L) / t: |dz| |Ws| (dx_mid), |dz|^T |x| (dWs), sum |dz| (dbs) and
sum |dz| |l| (dt).  Every bound has an absolute floor of 1e-37, under the smallest normal fp32 (the softmax weights of
far-off slices underflow to subnormals).  TAU below: the worst value measured on the MI355X over the kernel cases of this file, and the
bound (<= 4x that)."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_l2
from elementwise_check import check_products, poisoned

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENGINES = ("f32", "split", "bf16")
G9 = os.path.join(GOLDEN, "G9_encoder.npz")
TAU = {             # MI355X worst |got - ref| / scale over the kernel cases below in the comment; bound <= 4x that
    "sw": 7e-7,         # 1.9e-7  slice weights
    "dx": 9e-7,         # 2.4e-7  slice-weight backward, dx_mid
    "dws": 4e-7,        # 1.1e-7  dWs
    "dbs": 4e-7,        # 1.1e-7  dbs
    "dt": 9e-8,         # 2.3e-8  dtemperature
    "y": 1.6e-6,        # 4.2e-7  de-slice with explicit weights
    "dcode": 9e-7,      # 2.5e-7  its code gradient
    "dw": 1.2e-6,       # 3.2e-7  its weight gradient
}


def _check(got, ref, scale, key, label):
    # abs_floor: below the smallest normal fp32 (softmax weights of far-off slices underflow to subnormals)
    check_products(got, ref, scale, TAU[key], abs_floor=1e-37, label=label)


def _r(rng, *shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))


KERNEL_CASES = []     # (B, N, heads, D, M): every M x D, N in {1, 30, 4113}, B in {1, 3}
for _i, (_M, _D) in enumerate([(m, d) for m in (8, 32, 64, 128) for d in (8, 16, 32, 64)]):
    _N = (1, 30, 4113)[_i % 3]
    KERNEL_CASES.append(((1, 3)[_i % 2], _N, 2, _D, _M))
    if _N != 4113:
        KERNEL_CASES.append(((3, 1)[_i % 2], 4113, 2, _D, _M))
KERNEL_CASES += [(3, 1, 4, 16, 32), (1, 30, 8, 8, 8), (3, 30, 4, 32, 100), (2, 257, 2, 16, 13)]
IDS = [f"B{b}_N{n}_h{h}_D{d}_M{m}" for b, n, h, d, m in KERNEL_CASES]


def _slice_operands(B, N, heads, D, M, seed):
    rng = np.random.default_rng(seed)
    C = heads * D
    xf = _r(rng, B, N, 2 * C)                         # [x_mid | fx_mid]: x_mid is a view of row pitch 2C
    ws = _r(rng, M, D, scale=D ** -0.5)
    bs = _r(rng, M, scale=0.1)
    temp = torch.tensor(np.resize([0.03, 0.5, 7.0, 0.25, 1.5, 0.1, 5.0, 0.8], heads).astype(np.float32))
    dsw = _r(rng, B, heads, N, M)
    return xf, ws, bs, temp, dsw


def _slice_ref(xm, ws, bs, temp, dsw):
    """fp64 sw, the gradients, and the scales of the module docstring."""
    B, N, C = xm.shape
    heads = temp.numel()
    M, D = ws.shape
    x = xm.double().reshape(B, N, heads, D).permute(0, 2, 1, 3).clone().requires_grad_(True)
    W, b = ws.double().clone().requires_grad_(True), bs.double().clone().requires_grad_(True)
    t = temp.double().clone().requires_grad_(True)
    tc = t.clamp(0.1, 5.0).view(1, heads, 1, 1)
    logit = (x @ W.t() + b) / tc
    sw = torch.softmax(logit, -1)
    sw.backward(dsw.double())
    with torch.no_grad():
        L = (x.abs() @ W.abs().t() + b.abs()) / tc
        Lmax = L.amax(-1, keepdim=True)
        sw_scale = sw * (1 + L + Lmax)
        g = dsw.double()
        dz = sw * (g.abs() + (sw * g).sum(-1, keepdim=True).abs()) * (1 + Lmax) / tc
        dx_scale = (dz @ W.abs()).permute(0, 2, 1, 3).reshape(B, N, C)
        dws_scale = torch.einsum("bhnm,bhnd->md", dz, x.abs())
        dbs_scale = dz.sum((0, 1, 2))
        dt_scale = (dz * logit.abs()).sum((0, 2, 3))
    dx = x.grad.permute(0, 2, 1, 3).reshape(B, N, C)
    return (sw.detach(), sw_scale), (dx, dx_scale), (W.grad, dws_scale), (b.grad, dbs_scale), (t.grad, dt_scale)


@pytest.mark.parametrize("B,N,heads,D,M", KERNEL_CASES, ids=IDS)
def test_slice_weights_kernels_elementwise(B, N, heads, D, M):
    from transformerbasednavierstokesolver_amd import ops
    xf, ws, bs, temp, dsw = _slice_operands(B, N, heads, D, M, B * 7 + N + D * 3 + M)
    C = heads * D
    refs = _slice_ref(xf[:, :, :C], ws, bs, temp, dsw)
    xg, wsg, bsg, tg, dswg = (t.to(DEV) for t in (xf, ws, bs, temp, dsw))
    xm = xg[:, :, :C]                                   # ldx = 2C
    tag = f"B={B} N={N} heads={heads} D={D} M={M}"
    sw = poisoned(ops.slice_weights_fwd, xm, wsg, bsg, tg, heads)
    _check(sw.cpu(), *refs[0], "sw", tag + " slice weights")
    dxm, dws, dbs, dt = poisoned(ops.slice_weights_bwd, xm, wsg, bsg, tg, dswg)
    for got, (ref, sc), key in zip((dxm, dws, dbs, dt), refs[1:], ("dx", "dws", "dbs", "dt")):
        _check(got.cpu(), ref, sc, key, f"{tag} {key}")
    # no data gradient: the parameter gradients alone, identical bits
    none, dws2, dbs2, dt2 = ops.slice_weights_bwd(xm, wsg, bsg, tg, dswg, need_dx=False)
    assert none is None and torch.equal(dws2, dws) and torch.equal(dbs2, dbs) and torch.equal(dt2, dt)
    # accumulate = 1 into existing buffers
    into = tuple(torch.full_like(t, 0.5) for t in (dws, dbs, dt))
    ops.slice_weights_bwd(xm, wsg, bsg, tg, dswg, need_dx=False, into=into)
    for a, f in zip(into, (dws, dbs, dt)):
        torch.testing.assert_close(a, f + 0.5, rtol=1e-6, atol=1e-6)


def test_slice_weights_empty_batch():
    from transformerbasednavierstokesolver_amd import ops
    xf, ws, bs, temp, dsw = (t.to(DEV) for t in _slice_operands(1, 30, 4, 8, 8, 5))
    x0, d0 = xf[:0, :, :32], dsw[:0].contiguous()
    assert ops.slice_weights_fwd(x0, ws, bs, temp, 4).shape == (0, 4, 30, 8)
    dx, dws, dbs, dt = poisoned(ops.slice_weights_bwd, x0, ws, bs, temp, d0, need_dx=False)
    assert dx is None and all(torch.count_nonzero(t) == 0 for t in (dws, dbs, dt))


@pytest.mark.parametrize("B,N,heads,D,M", KERNEL_CASES, ids=IDS)
def test_deslice_weights_kernels_elementwise(B, N, heads, D, M):
    from transformerbasednavierstokesolver_amd import ops
    rng = np.random.default_rng(B * 11 + N + D * 5 + M)
    C = heads * D
    code, w, dy = _r(rng, B, heads, M, D), _r(rng, B, heads, N, M), _r(rng, B, N, C)
    cd, wd, dyd = code.double(), w.double(), dy.double().reshape(B, N, heads, D).permute(0, 2, 1, 3)
    y_ref = torch.einsum("bhgc,bhng->bhnc", cd, wd).permute(0, 2, 1, 3).reshape(B, N, C)
    y_sc = torch.einsum("bhgc,bhng->bhnc", cd.abs(), wd.abs()).permute(0, 2, 1, 3).reshape(B, N, C)
    dcode_ref, dcode_sc = wd.transpose(2, 3) @ dyd, wd.abs().transpose(2, 3) @ dyd.abs()
    dw_ref, dw_sc = dyd @ cd.transpose(2, 3), dyd.abs() @ cd.abs().transpose(2, 3)
    cg, wg, dyg = code.to(DEV), w.to(DEV), dy.to(DEV)
    tag = f"B={B} N={N} heads={heads} D={D} M={M}"
    y = poisoned(ops.deslice_weights_fwd, cg, wg)
    _check(y.cpu(), y_ref, y_sc, "y", tag + " de-slice")
    dcode, dw = poisoned(ops.deslice_weights_bwd, cg, wg, dyg)
    _check(dcode.cpu(), dcode_ref, dcode_sc, "dcode", tag + " dcode")
    _check(dw.cpu(), dw_ref, dw_sc, "dw", tag + " dw")
    # NULL-output modes: a frozen encoder's weights, a code without gradient
    dc_only, none = poisoned(ops.deslice_weights_bwd, cg, wg, dyg, need_dw=False)
    assert none is None and torch.equal(dc_only, dcode)
    none, dw_only = poisoned(ops.deslice_weights_bwd, cg, wg, dyg, need_dcode=False)
    assert none is None and torch.equal(dw_only, dw)


# ---------------------------------------------------------------------------------------------- vs the reference (G9)
@pytest.fixture(scope="module")
def g9():
    return np.load(G9)


def _regenerate(g9, pre):
    from test_encoder_host import regenerate
    return regenerate(g9, pre)


def _rel(g9, key, got):
    """rel-L2 against the fixture entry (whole tensor, or its strided sample and norm)."""
    got = got.detach().double().cpu()
    if key in g9.files:
        return rel_l2(got.reshape(-1), torch.from_numpy(g9[key]).double().reshape(-1))
    stride, want = int(g9[key + ".stride"]), torch.from_numpy(g9[key + ".sample"]).double()
    s = got.reshape(-1)[::stride][:want.numel()]
    nrm = float(g9[key + ".norm"])
    return max(rel_l2(s, want), abs(float(got.norm()) - nrm) / nrm)


def _grad_tol(engine, name):
    """The G8 tests' tolerances on the f32 and split engines.  On the one-term bf16 engine the gradients get 6e-2
    instead of 3e-2: attn_m32 (temperature 0.03 clamped to 0.1, the sharpest softmax of the fixture) measured 3.2e-2 for
    the temperature and to_k gradients on the MI355X."""
    if engine == "bf16":
        return 6e-2
    return 2e-3 if ("to_q" in name or "to_k" in name) else 1e-4


def _fwd_tol(engine):
    return 3e-2 if engine == "bf16" else 1e-5


def _model(g9, pre, engine):
    from transformerbasednavierstokesolver_amd.model.Transolver_Structured_Mesh2D_Encoder import Model
    m = Model(**json.loads(str(g9[pre + "config"])))
    m.load_state_dict(_regenerate(g9, pre), strict=True)
    return m.to(DEV).set_engine(engine)


def _t(g9, key):
    return torch.from_numpy(g9[key]).to(DEV) if key in g9.files else None


def _check_grads(g9, pre, m, engine):
    none = set(json.loads(str(g9[pre + "no_grad"])))
    for k, p in m.named_parameters():
        if k in none:
            assert p.grad is None, k                     # the reference has no gradient there, and neither may we
            continue
        e = _rel(g9, pre + "grad." + k, p.grad)
        assert e <= _grad_tol(engine, k), (k, e)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("variant", ["up", "nofx", "time"])
def test_full_model_matches_reference(g9, variant, engine):
    from transformerbasednavierstokesolver_amd.utils.testloss import TestLoss
    pre = f"tiny_{variant}."
    m = _model(g9, pre, engine)
    x, fx, y, T = _t(g9, pre + "x"), _t(g9, pre + "fx"), _t(g9, pre + "y"), _t(g9, pre + "T")
    B = x.shape[0]
    pred = m(x, fx, T=T)
    loss = TestLoss(size_average=False)(pred.reshape(B, -1), y.reshape(B, -1))
    loss.backward()
    assert _rel(g9, pre + "pred", pred) <= _fwd_tol(engine)
    assert abs(float(loss.detach()) - float(g9[pre + "loss"])) <= _fwd_tol(engine) * abs(float(g9[pre + "loss"]))
    _check_grads(g9, pre, m, engine)
    if T is None:      # forward(x, fx) with T = None is decode(encode(x, fx)), bit for bit
        with torch.no_grad():
            assert torch.equal(m(x, fx), m.decode(m.encode(x, fx)))


@pytest.mark.parametrize("engine", ENGINES)
def test_stateful_sequence_matches_reference(g9, engine):
    from transformerbasednavierstokesolver_amd.utils.testloss import TestLoss
    pre = "seq."
    m = _model(g9, pre, engine)
    x, fx, y = _t(g9, pre + "x"), _t(g9, pre + "fx"), _t(g9, pre + "y")
    B = x.shape[0]
    tol = _fwd_tol(engine)
    with torch.no_grad():
        code = m.encode(x, fx)
        assert _rel(g9, pre + "code", code) <= tol
        s0 = m.get_attention_slice()
        assert m.get_attention_slice() is s0                 # the cached tensor object itself
        assert _rel(g9, pre + "slice0", s0) <= tol
        assert _rel(g9, pre + "y1", m.decode(code)) <= tol
        assert _rel(g9, pre + "slice1", m.get_attention_slice()) <= tol
        assert _rel(g9, pre + "y2", m.decode(code)) <= tol            # P(P(sw))
        assert _rel(g9, pre + "slice2", m.get_attention_slice()) <= tol
        S = _t(g9, pre + "S")
        keep = S.clone()
        m.set_attention_slice(S)
        assert m.get_attention_slice() is S
        assert _rel(g9, pre + "y3", m.decode(code)) <= tol
        assert torch.equal(S, keep)                          # decode reassigns the attribute, never writes into S
        assert m.get_attention_slice() is not S
    with pytest.raises(AttributeError):
        m.get_attention_code()
    # gradients of a loss on y1: every parameter and the code
    code = m.encode(x, fx)
    code.retain_grad()
    loss = TestLoss(size_average=False)(m.decode(code).reshape(B, -1), y.reshape(B, -1))
    loss.backward()
    assert abs(float(loss.detach()) - float(g9[pre + "loss1"])) <= tol * float(g9[pre + "loss1"])
    assert _rel(g9, pre + "dcode", code.grad) <= _grad_tol(engine, "code")
    _check_grads(g9, pre, m, engine)
    # frozen encoder (SequenSolver): only the code has a gradient
    for p in m.parameters():
        p.requires_grad_(False)
        p.grad = None
    with torch.no_grad():
        code = m.encode(x, fx)
    code = code.clone().requires_grad_(True)
    TestLoss(size_average=False)(m.decode(code).reshape(B, -1), y.reshape(B, -1)).backward()
    assert _rel(g9, pre + "dcode_frozen", code.grad) <= _grad_tol(engine, "code")
    assert all(p.grad is None for p in m.parameters())
    # a caller-supplied slice tensor that requires grad receives one (through project_slice)
    S2 = _t(g9, pre + "S").clone().requires_grad_(True)
    m.set_attention_slice(S2)
    m.decode(code.detach()).sum().backward()
    assert S2.grad is not None and bool(torch.isfinite(S2.grad).all()) and torch.count_nonzero(S2.grad) > 0


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("case", ["m32", "m128"])
def test_attention_module_matches_reference(g9, case, engine):
    from transformerbasednavierstokesolver_amd.model.Physics_Attention import \
        Physics_Attention_Structured_Mesh_2D_Auto_Encoder as Attn
    pre = f"attn_{case}."
    H, W, C, heads, M, B = (int(v) for v in g9[pre + "geom"])
    a = Attn(C, heads=heads, dim_head=C // heads, slice_num=M, H=H, W=W)
    a.load_state_dict(_regenerate(g9, pre), strict=True)
    a = a.to(DEV)
    a.engine = {"f32": 0, "split": 1, "bf16": 2}[engine]
    rng = np.random.default_rng(int(g9[pre + "seed"]) + 100)
    x = rng.standard_normal((B, H * W, C)).astype(np.float32)
    gy = rng.standard_normal((B, H * W, C)).astype(np.float32)
    assert np.sum(x, dtype=np.float64) == float(g9[pre + "x.sum"]) and np.sum(gy, dtype=np.float64) == float(g9[pre + "gy.sum"])
    xt = torch.from_numpy(x).to(DEV).requires_grad_(True)
    code = a.encode(xt, cache_slice=True)
    sw = a.slice_weights
    y = a.reconstruct_fx(code) + a.decode(code)
    y.backward(torch.from_numpy(gy).to(DEV))
    assert _rel(g9, pre + "code", code) <= _fwd_tol(engine)
    assert _rel(g9, pre + "sw", sw) <= _fwd_tol(engine)
    assert _rel(g9, pre + "y", y) <= _fwd_tol(engine)
    assert _rel(g9, pre + "dx", xt.grad) <= _grad_tol(engine, "dx")
    for k, p in a.named_parameters():
        e = _rel(g9, pre + "grad." + k, p.grad)
        assert e <= _grad_tol(engine, k), (k, e)


def test_flat_bucket_fused_adamw_and_autoencoder_steps(g9):
    from transformerbasednavierstokesolver_amd import harness
    from transformerbasednavierstokesolver_amd.ddp import FlatGradSync
    from transformerbasednavierstokesolver_amd.optim import FusedAdamW
    from transformerbasednavierstokesolver_amd.utils.testloss import TestLoss
    pre = "tiny_up."
    x, fx, y = _t(g9, pre + "x"), _t(g9, pre + "fx"), _t(g9, pre + "y")
    B = x.shape[0]

    def run(m):
        return TestLoss(size_average=False)(m(x, fx).reshape(B, -1), y.reshape(B, -1))
    m = _model(g9, pre, "split")
    run(m).backward()
    plain = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    m2 = _model(g9, pre, "split")
    sync = FlatGradSync(m2.parameters())       # before the backward: the kernels add straight into the bucket
    run(m2).backward()
    sync()
    for k, p in m2.named_parameters():
        if k in plain:
            assert p.grad.data_ptr() == sync.views[sync.index_of(p)].data_ptr()
            assert rel_l2(p.grad, plain[k]) <= 1e-6, k
        else:
            assert p.grad is None, k
    # three auto_encoder.py iterations with FusedAdamW against the reference's torch.optim.AdamW losses
    pre = "adamw."
    hyper = json.loads(str(g9[pre + "hyper"]))
    mt = _model(g9, pre, "f32")
    opt = FusedAdamW(mt.parameters(), lr=hyper["lr"], weight_decay=hyper["weight_decay"], max_grad_norm=hyper["clip"])
    frozen = {k: p.detach().clone() for k, p in mt.named_parameters() if k.startswith("blocks.0.Attn.project_slice")}
    assert len(frozen) == 2
    xa, fxa = _t(g9, pre + "x"), _t(g9, pre + "fx")
    losses = [float(harness.autoencoder_train_step(mt, opt, None, xa, fxa, grad_sync=opt.sync))
              for _ in range(hyper["steps"])]
    np.testing.assert_allclose(losses, g9[pre + "losses"], rtol=2e-5)
    for k, p in mt.named_parameters():
        if k in frozen:      # never had a gradient: no weight decay lands on it either
            assert torch.equal(p.detach(), frozen[k]), k
