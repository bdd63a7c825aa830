"""Structured 3-D mesh family on the MI355X: the 27-tap implicit-GEMM conv (pa2d_conv3x3x3x2_*) element by element against
CPU fp64 torch.nn.functional.conv3d and its autograd, against the 3x3 conv at depth 1, at the real size against fp64
direct sums; the attention module and the full model against the reference's fp64 outputs (tests/golden/G8_structured3d.npz,
tools/make_golden_3d.py); the training plumbing (flat gradient bucket, FusedAdamW, use_checkpoint).

Per-element bounds: TAU[(engine, "fwd" | "wgrad")] of elementwise_check.py for the fp32-accurate engines, the same values
the 3x3 conv is held to.  The `bf16` engine (one bf16 term on fp32 storage: both operands rounded to bf16, up to 2^-8 of
|x| |w| per product) has no TAU entry; BF16_TAU below is TAU[("bf16s", "fwd")], the bound of the other one-term engine."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, rel_l2
from elementwise_check import TAU, check_products, poisoned

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENGINES = ("f32", "split", "bf16")
BF16_TAU = TAU[("bf16s", "fwd")]
G8 = os.path.join(GOLDEN, "G8_structured3d.npz")


def _tau(engine, fam):
    return BF16_TAU if engine == "bf16" else TAU[(engine, fam)]


def _r(rng, *shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))


def _conv3d(x, w, b, H, W, D):
    """[B, N, Cin] (n = (h*W + w)*D + d) -> [B, N, Cout]: the reference's reshape / permute around nn.Conv3d."""
    B, N, C = x.shape
    xi = x.reshape(B, H, W, D, C).permute(0, 4, 1, 2, 3)
    y = F.conv3d(xi, w, b, padding=1)
    return y.permute(0, 2, 3, 4, 1).reshape(B, N, -1)


def _conv_refs(x, wx, bx, wf, bf, dout, H, W, D):
    """(out, dxn, dwx, dbx, dwf, dbf) of the fused pair in CPU fp64, and the same on absolute values (the scales)."""
    def run(*ts):
        ts = [t.detach().double().cpu().clone().requires_grad_(True) for t in ts[:5]] + [ts[5].double().cpu()]
        out = torch.cat([_conv3d(ts[0], ts[1], ts[2], H, W, D), _conv3d(ts[0], ts[3], ts[4], H, W, D)], -1)
        out.backward(ts[5])
        return (out.detach(),) + tuple(t.grad for t in ts[:5])
    return run(x, wx, bx, wf, bf, dout), run(x.abs(), wx.abs(), bx.abs(), wf.abs(), bf.abs(), dout.abs())


def _operands(seed, B, H, W, D, C):
    rng = np.random.default_rng(seed)
    N = H * W * D
    x, dout = _r(rng, B, N, C), _r(rng, B, N, 2 * C)
    wx, wf = _r(rng, C, C, 3, 3, 3, scale=(27 * C) ** -0.5), _r(rng, C, C, 3, 3, 3, scale=(27 * C) ** -0.5)
    bx, bf = 0.1 * _r(rng, C), 0.1 * _r(rng, C)
    return x, wx, bx, wf, bf, dout


CONV_CASES = [  # B, H, W, D, C: degenerate extents, 1x1x1, rows (B*H*W*D) never a multiple of a tile
    (2, 4, 5, 3, 16),
    (3, 4, 5, 3, 32),
    (2, 1, 6, 5, 64),
    (2, 3, 1, 7, 32),
    (3, 1, 1, 1, 32),
    (2, 8, 8, 8, 64),
    (3, 8, 8, 8, 32),
    (2, 5, 7, 9, 64),
]


@pytest.mark.parametrize("B,H,W,D,C", CONV_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}x{c[3]}x{c[4]}" for c in CONV_CASES])
def test_conv3d_elementwise(B, H, W, D, C):
    from transformerbasednavierstokesolver_amd import ops
    x, wx, bx, wf, bf, dout = _operands(B * 1000 + H * 100 + W * 10 + D + C, B, H, W, D, C)
    (out_r, dx_r, dwx_r, dbx_r, dwf_r, dbf_r), (out_s, dx_s, dwx_s, dbx_s, dwf_s, dbf_s) = \
        _conv_refs(x, wx, bx, wf, bf, dout, H, W, D)
    xg, wxg, bxg, wfg, bfg, dg = (t.to(DEV) for t in (x, wx, bx, wf, bf, dout))
    for engine in ENGINES:
        tag = f"[{engine}] conv3d B={B} H={H} W={W} D={D} C={C}"
        out = poisoned(ops.conv3x3x3x2_fwd, xg, wxg, bxg, wfg, bfg, H, W, D, engine=engine)
        check_products(out.cpu(), out_r, out_s, _tau(engine, "fwd"), label=tag + " forward")
        dxn, dwx, dbx, dwf, dbf = poisoned(ops.conv3x3x3x2_bwd, dg, xg, wxg, wfg, H, W, D, engine=engine)
        check_products(dxn.cpu(), dx_r, dx_s, _tau(engine, "fwd"), label=tag + " data gradient")
        for got, ref, sc, name in ((dwx, dwx_r, dwx_s, "dwx"), (dwf, dwf_r, dwf_s, "dwf")):
            check_products(got.cpu().reshape(C, -1), ref.reshape(C, -1), sc.reshape(C, -1), _tau(engine, "wgrad"),
                           label=f"{tag} {name} [co, ci*27+tap]")
        check_products(dbx.cpu(), dbx_r, dbx_s, _tau(engine, "wgrad"), label=tag + " dbx")
        check_products(dbf.cpu(), dbf_r, dbf_s, _tau(engine, "wgrad"), label=tag + " dbf")


def test_conv3d_real_size_split_sampled():
    """32^3, C = 256, B = 1 on the split engine (K = 6912 forward, 13 824 data gradient): 96 sampled output rows (all 512
    columns) and 16 sampled output channels of dWx / dWf (all [C_in, 27] entries) against fp64 direct sums."""
    from transformerbasednavierstokesolver_amd import ops
    H = W = D = 32
    C, B = 256, 1
    N = H * W * D
    x, wx, bx, wf, bf, dout = _operands(7, B, H, W, D, C)
    xg, wxg, bxg, wfg, bfg, dg = (t.to(DEV) for t in (x, wx, bx, wf, bf, dout))
    out = ops.conv3x3x3x2_fwd(xg, wxg, bxg, wfg, bfg, H, W, D, engine="split").cpu().double()[0]
    _, dwx, dbx, dwf, dbf = ops.conv3x3x3x2_bwd(dg, xg, wxg, wfg, H, W, D, need_dx=False, engine="split")
    xp = F.pad(x.double()[0].reshape(H, W, D, C), (0, 0, 1, 1, 1, 1, 1, 1))     # zero padding on all six faces
    taps = [(kh, kw, kd) for kh in range(3) for kw in range(3) for kd in range(3)]      # t = kh*9 + kw*3 + kd

    def shifted(t):      # x at the tap's neighbour of every point, [N, C] (zero outside the mesh)
        kh, kw, kd = taps[t]
        return xp[kh:kh + H, kw:kw + W, kd:kd + D].reshape(N, C)
    rng = np.random.default_rng(8)
    rows = np.unique(np.concatenate([rng.integers(0, N, 88), [0, N - 1, D - 1, W * D - 1, (H - 1) * W * D, 1234, 31 * 32 + 5,
                                                                 N // 2]]))
    patch = torch.stack([shifted(t)[rows] for t in range(27)], 1).reshape(len(rows), 27 * C)   # [rows, tap*C + ci]
    wcat = torch.cat([wx, wf], 0).double().permute(0, 2, 3, 4, 1).reshape(2 * C, 27 * C)     # [co, tap*C + ci]
    bcat = torch.cat([bx, bf]).double()
    check_products(out[rows], patch @ wcat.t() + bcat, patch.abs() @ wcat.abs().t() + bcat.abs(), TAU[("split", "fwd")],
                   label="[split] conv3d 32^3 C=256 sampled output rows")
    cos = np.sort(rng.choice(2 * C, 16, replace=False))
    dsel = dout.double()[0][:, cos]                                                          # [N, 16]
    ref = torch.stack([dsel.t() @ shifted(t) for t in range(27)], 2)                        # [16, C_in, 27]
    sc = torch.stack([dsel.abs().t() @ shifted(t).abs() for t in range(27)], 2)
    dw = torch.cat([dwx, dwf], 0).cpu().double().reshape(2 * C, C, 27)[cos]
    check_products(dw.reshape(16, -1), ref.reshape(16, -1), sc.reshape(16, -1), TAU[("split", "wgrad")],
                   label="[split] conv3d 32^3 C=256 dW, 16 sampled output channels")
    db = torch.cat([dbx, dbf]).cpu().double()
    check_products(db, dout.double()[0].sum(0), dout.double()[0].abs().sum(0), TAU[("split", "wgrad")],
                   label="[split] conv3d 32^3 C=256 bias gradients")


@pytest.mark.parametrize("engine", ENGINES)
def test_conv3d_depth1_equals_3x3_conv(engine):
    """D = 1 with only the kd = 1 taps non-zero: the 27-tap conv is the 9-tap conv of pa2d_conv3x3x2_*; the gradients of
    the kd = 0 / 2 taps read only the zero padding and are exactly 0."""
    from transformerbasednavierstokesolver_amd import ops
    B, H, W, C = 2, 12, 20, 64
    x, w3x, bx, w3f, bf, dout = _operands(11, B, H, W, 1, C)
    mask = torch.zeros(3)
    mask[1] = 1.0
    w3x, w3f = w3x * mask, w3f * mask
    w2x, w2f = w3x[..., 1].contiguous(), w3f[..., 1].contiguous()
    g = lambda *ts: [t.to(DEV) for t in ts]
    xg, w3xg, w3fg, w2xg, w2fg, bxg, bfg, dg = g(x, w3x, w3f, w2x, w2f, bx, bf, dout)
    (o2_s, dx2_s, dw2x_s, _, dw2f_s, _) = _conv_refs(x.abs(), w3x.abs(), bx.abs(), w3f.abs(), bf.abs(), dout.abs(),
                                                     H, W, 1)[0]
    o3 = ops.conv3x3x3x2_fwd(xg, w3xg, bxg, w3fg, bfg, H, W, 1, engine=engine)
    o2 = ops.conv3x3x2_fwd(xg, w2xg, bxg, w2fg, bfg, H, W, engine=engine)
    check_products(o3.cpu(), o2.cpu(), o2_s, _tau(engine, "fwd"), label=f"[{engine}] depth-1 forward vs 3x3 conv")
    d3 = ops.conv3x3x3x2_bwd(dg, xg, w3xg, w3fg, H, W, 1, engine=engine)
    d2 = ops.conv3x3x2_bwd(dg, xg, w2xg, w2fg, H, W, engine=engine)
    check_products(d3[0].cpu(), d2[0].cpu(), dx2_s, _tau(engine, "fwd"), label=f"[{engine}] depth-1 data gradient")
    for i, sc in ((1, dw2x_s), (3, dw2f_s)):
        g3 = d3[i].cpu()
        assert torch.count_nonzero(g3[..., 0]) == 0 and torch.count_nonzero(g3[..., 2]) == 0
        check_products(g3[..., 1].reshape(C, -1), d2[i].cpu().reshape(C, -1), sc[..., 1].reshape(C, -1),
                       _tau(engine, "wgrad"), label=f"[{engine}] depth-1 weight gradient {i}")
    colsum = dout.abs().double().sum((0, 1))
    for i, sc in ((2, colsum[:C]), (4, colsum[C:])):
        check_products(d3[i].cpu(), d2[i].cpu(), sc, _tau(engine, "wgrad"), label=f"[{engine}] depth-1 bias gradient {i}")


@pytest.mark.parametrize("engine", ENGINES)
def test_conv3d_accumulate_empty_batch_and_frozen_pack(engine):
    from transformerbasednavierstokesolver_amd import ops
    B, H, W, D, C = 2, 4, 5, 3, 32
    ts = [t.to(DEV) for t in _operands(5, B, H, W, D, C)]
    x, wx, bx, wf, bf, dout = ts
    out = ops.conv3x3x3x2_fwd(x, wx, bx, wf, bf, H, W, D, engine=engine)
    fresh = ops.conv3x3x3x2_bwd(dout, x, wx, wf, H, W, D, engine=engine)
    # accumulate = 1: the kernels add into the given buffers
    seeds = [torch.full_like(t, 0.25) for t in fresh[1:]]
    into = [s.clone() for s in seeds]
    acc = ops.conv3x3x3x2_bwd(dout, x, wx, wf, H, W, D, need_dx=False, engine=engine, into=tuple(into))
    assert acc[0] is None
    for got, s, f in zip(acc[1:], seeds, fresh[1:]):
        assert got.data_ptr() in [t.data_ptr() for t in into]
        torch.testing.assert_close(got, s + f, rtol=1e-6, atol=1e-6)
    # B = 0: forward is a no-op, the gradients are zero-filled (accumulate = 0) or left alone (accumulate = 1)
    x0, d0 = x[:0].contiguous(), dout[:0].contiguous()
    assert ops.conv3x3x3x2_fwd(x0, wx, bx, wf, bf, H, W, D, engine=engine).shape == (0, H * W * D, 2 * C)
    z = poisoned(ops.conv3x3x3x2_bwd, d0, x0, wx, wf, H, W, D, need_dx=False, engine=engine)
    assert all(torch.count_nonzero(t) == 0 for t in z[1:])
    kept = [s.clone() for s in seeds]
    ops.conv3x3x3x2_bwd(d0, x0, wx, wf, H, W, D, need_dx=False, engine=engine, into=tuple(kept))
    assert all(torch.equal(a, b) for a, b in zip(kept, seeds))
    # a pack made once in a weights_frozen() scope gives the same bits as the pack made inside the call
    with ops.weights_frozen() as scope:
        out_f = ops.conv3x3x3x2_fwd(x, wx, bx, wf, bf, H, W, D, engine=engine)
        bwd_f = ops.conv3x3x3x2_bwd(dout, x, wx, wf, H, W, D, engine=engine)
        # a 3x3 model of the same (B, H, W, C) in the same scope gets its own pack
        ops.conv3x3x2_fwd(x[:, :H * W].contiguous(), wx[..., 1].contiguous(), bx, wf[..., 1].contiguous(), bf, H, W,
                          engine=engine)
        depths = sorted(str(k[5]) for k in scope.packs)
        assert "3" in depths and "None" in depths
    assert torch.equal(out_f, out)
    assert all(torch.equal(a, b) for a, b in zip(bwd_f, fresh))


def test_conv3d_refuses_bf16_storage():
    from transformerbasednavierstokesolver_amd import ops
    x = torch.zeros(1, 8, 32, device=DEV, dtype=torch.bfloat16)
    w = torch.zeros(32, 32, 3, 3, 3, device=DEV)
    b = torch.zeros(32, device=DEV)
    with pytest.raises(NotImplementedError):
        ops.conv3x3x3x2_fwd(x, w, b, w, b, 2, 2, 2)
    with pytest.raises(NotImplementedError):
        ops.conv3x3x3x2_fwd(x.float(), w, b, w, b, 2, 2, 2, engine="bf16s")


# ---------------------------------------------------------------------------------------------- vs the reference (G8)
@pytest.fixture(scope="module")
def g8():
    return np.load(G8)


def _regenerate(g8, pre):
    from test_structured3d_host import regenerate
    return regenerate(g8, pre)


def _rel(g8, key, got):
    """rel-L2 of `got` against the fixture entry (whole tensor, or its strided sample and norm); no entry: the reference
    has no gradient there (the placeholder when fx is given), and neither may we."""
    if key not in g8.files and key + ".sample" not in g8.files:
        assert got is None or torch.count_nonzero(got) == 0, key
        return 0.0
    got = got.detach().double().cpu()
    if key in g8.files:
        return rel_l2(got.reshape(-1), torch.from_numpy(g8[key]).double().reshape(-1))
    stride, want = int(g8[key + ".stride"]), torch.from_numpy(g8[key + ".sample"]).double()
    s = got.reshape(-1)[::stride][:want.numel()]
    nrm = float(g8[key + ".norm"])
    return max(rel_l2(s, want), abs(float(got.norm()) - nrm) / nrm)


def _grad_tol(engine, name):
    if engine == "bf16":
        return 3e-2
    return 2e-3 if ("to_q" in name or "to_k" in name) else 1e-4


def _fwd_tol(engine):
    return 3e-2 if engine == "bf16" else 1e-5


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("case", ["8x8x8", "1x6x5", "3x1x7"])
def test_attention_module_matches_reference(g8, case, engine):
    from transformerbasednavierstokesolver_amd.model.Physics_Attention import Physics_Attention_Structured_Mesh_3D
    pre = f"attn_{case}."
    H, W, D, C, heads, M, B = (int(v) for v in g8[pre + "geom"])
    a = Physics_Attention_Structured_Mesh_3D(C, heads=heads, dim_head=C // heads, slice_num=M, H=H, W=W, D=D)
    a.load_state_dict(_regenerate(g8, pre), strict=True)
    a = a.to(DEV)
    a.engine = {"f32": 0, "split": 1, "bf16": 2}[engine]
    rng = np.random.default_rng(int(g8[pre + "seed"]) + 100)
    x = rng.standard_normal((B, H * W * D, C)).astype(np.float32)
    gy = rng.standard_normal((B, H * W * D, C)).astype(np.float32)
    assert np.sum(x, dtype=np.float64) == float(g8[pre + "x.sum"]) and np.sum(gy, dtype=np.float64) == float(g8[pre + "gy.sum"])
    xt = torch.from_numpy(x).to(DEV).requires_grad_(True)
    y = a(xt)
    y.backward(torch.from_numpy(gy).to(DEV))
    assert _rel(g8, pre + "y", y) <= _fwd_tol(engine)
    assert _rel(g8, pre + "dx", xt.grad) <= _grad_tol(engine, "dx")
    for k, p in a.named_parameters():
        e = _rel(g8, pre + "grad." + k, p.grad)
        assert e <= _grad_tol(engine, k), (k, e)


def _tiny(g8, variant, engine, checkpointing=False):
    from transformerbasednavierstokesolver_amd.model.Transolver_Structured_Mesh_3D import Model
    from transformerbasednavierstokesolver_amd.utils.testloss import TestLoss
    pre = f"tiny_{variant}."
    cfg = json.loads(str(g8[pre + "config"]))
    m = Model(**cfg)
    m.load_state_dict(_regenerate(g8, pre), strict=True)
    m = m.to(DEV).set_engine(engine)
    m.use_checkpoint = checkpointing
    t = lambda k: torch.from_numpy(g8[pre + k]).to(DEV) if pre + k in g8.files else None
    x, fx, y, T = t("x"), t("fx"), t("y"), t("T")
    B = x.shape[0]
    pred = m(x, fx, T=T)
    loss = TestLoss(size_average=False)(pred.reshape(B, -1), y.reshape(B, -1))
    return m, pre, pred, loss


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("variant", ["up", "nofx", "time"])
def test_full_model_matches_reference(g8, variant, engine):
    m, pre, pred, loss = _tiny(g8, variant, engine)
    loss.backward()
    assert _rel(g8, pre + "pred", pred) <= _fwd_tol(engine)
    assert abs(float(loss.detach()) - float(g8[pre + "loss"])) <= _fwd_tol(engine) * abs(float(g8[pre + "loss"]))
    for k, p in m.named_parameters():
        e = _rel(g8, pre + "grad." + k, p.grad)
        assert e <= _grad_tol(engine, k), (k, e)


def test_flat_bucket_fused_adamw_and_checkpointing(g8):
    from transformerbasednavierstokesolver_amd import harness
    from transformerbasednavierstokesolver_amd.ddp import FlatGradSync
    from transformerbasednavierstokesolver_amd.model.Transolver_Structured_Mesh_3D import Model
    from transformerbasednavierstokesolver_amd.optim import FusedAdamW
    # gradients through the flat bucket at world size 1 (the kernels' into= path) equal the plain ones
    m, _, _, loss = _tiny(g8, "up", "split")
    loss.backward()
    plain = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    m2, _, _, loss2 = _tiny(g8, "up", "split")
    sync = FlatGradSync(m2.parameters())       # before the backward: the kernels add straight into the bucket
    loss2.backward()
    sync()
    for k, p in m2.named_parameters():
        if k in plain:
            assert p.grad.data_ptr() == sync.views[sync.index_of(p)].data_ptr()
            assert rel_l2(p.grad, plain[k]) <= 1e-6, k
        else:                                   # unused parameter (the placeholder when fx is given): no gradient
            assert p.grad is None or torch.count_nonzero(p.grad) == 0, k
    # use_checkpoint: the blocks run under torch.utils.checkpoint, same gradients
    mc, _, _, lc = _tiny(g8, "up", "split", checkpointing=True)
    lc.backward()
    for k, p in mc.named_parameters():
        assert (p.grad is None) == (k not in plain), k
        if k in plain:
            assert rel_l2(p.grad, plain[k]) <= 1e-6, k
    # one training step with FusedAdamW
    torch.manual_seed(3)
    mt = Model(space_dim=3, n_layers=2, n_hidden=32, n_head=4, fun_dim=2, out_dim=1, slice_num=8, H=4, W=5, D=3).to(DEV)
    opt = FusedAdamW(mt.parameters(), lr=1e-3, weight_decay=1e-5, max_grad_norm=1.0)
    before = [p.detach().clone() for p in mt.parameters()]
    g = torch.Generator().manual_seed(4)
    xx, ff, yy = (torch.randn(2, 60, k, generator=g).to(DEV) for k in (3, 2, 2))
    loss, _ = harness.train_step(mt, opt, None, xx, ff, yy, grad_sync=opt.sync)
    assert torch.isfinite(loss)
    assert all(torch.isfinite(p).all() for p in mt.parameters())
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, mt.parameters()))
