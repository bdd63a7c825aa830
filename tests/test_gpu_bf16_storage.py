"""bf16-STORAGE path (BASELINE configs[2] "NS 64x64 bf16 ... DDP", configs[4] "Darcy ... bf16"):
activations, saved tensors and inter-kernel gradients are bf16 in HBM, parameters / statistics / accumulators fp32.

Stage tests feed the kernels bf16 tensors and compare with the fp64 oracle evaluated on THE SAME (bf16-rounded) values,
so what is measured is the kernel's own error: bf16 rounding of the stored outputs (2^-9 relative per element) and of the
weights inside the one-term bf16 MFMA.  Tolerance 1e-2 per stage; SURVEY 8c: full-model forward <= 3e-2 vs fp64 (the
reference under bf16 autocast is 1.4-1.6e-2)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-2
BF = torch.bfloat16


def _r(rng, *shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))


def _b(t):
    """bf16 tensor on the device + the double copy of exactly the values it holds"""
    tb = t.to(DEV).to(BF).contiguous()
    return tb, tb.double().cpu()


@pytest.mark.parametrize("rows,C", [(7, 32), (300, 64), (4096, 256)])
def test_layernorm_bf16(rows, C):
    from transformerbasednavierstokesolver_amd import ops
    from oracle import transolver_oracle as orc
    rng = np.random.default_rng(rows + C)
    (x, xd), (dy, dyd), (dres, dresd) = _b(_r(rng, rows, C) * 2 + 0.5), _b(_r(rng, rows, C)), _b(_r(rng, rows, C))
    g, b = 1 + 0.1 * _r(rng, C), 0.1 * _r(rng, C)
    xq = xd.clone().requires_grad_(True)
    gd, bd = g.double().requires_grad_(True), b.double().requires_grad_(True)
    yo = orc.layer_norm(xq, gd, bd)
    yo.backward(dyd)
    y, mean, rstd = ops.layernorm_fwd(x, g.to(DEV), b.to(DEV))
    assert y.dtype == BF and mean.dtype == torch.float32
    assert rel_l2(y, yo) < TOL
    dx, dg, db = ops.layernorm_bwd(dy, x, mean, rstd, g.to(DEV), dres)
    assert dx.dtype == BF and dg.dtype == torch.float32
    assert rel_l2(dx, xq.grad + dresd) < TOL
    assert rel_l2(dg, gd.grad) < 1e-4 and rel_l2(db, bd.grad) < 1e-4          # fp32 reductions of exact inputs


@pytest.mark.parametrize("M,N,K,act", [(60, 32, 32, "gelu"), (4096, 256, 256, "gelu"), (1000, 512, 64, None), (333, 96, 160, "silu"),
                                       (66001, 256, 256, "gelu"), (65536, 192, 128, None)])      # last two: row-panel kernel
def test_linear_bf16(M, N, K, act):
    from transformerbasednavierstokesolver_amd import ops
    from oracle import transolver_oracle as orc
    rng = np.random.default_rng(M + N + K)
    (x, xd), (res, resd), (dy, dyd) = _b(_r(rng, M, K)), _b(_r(rng, M, N)), _b(_r(rng, M, N))
    w, b = _r(rng, N, K, scale=K ** -0.5), 0.1 * _r(rng, N)
    pre = xd @ w.double().t() + b.double()
    yo = (orc._ACTS[act](pre) if act else pre) + resd
    y, pre_k = ops.linear_fwd(x, w.to(DEV), b.to(DEV), res=res, act=act, want_pre=True)
    assert y.dtype == BF and pre_k.dtype == BF
    assert rel_l2(y, yo) < TOL and rel_l2(pre_k, pre) < TOL
    dwk, dbk = ops.linear_bwd_weight(dy, x)
    assert dwk.dtype == torch.float32
    assert rel_l2(dwk, dyd.t() @ xd) < 1e-4 and rel_l2(dbk, dyd.sum(0)) < 1e-4      # exact bf16 products, fp32 sums
    acc_w, acc_b = torch.full_like(dwk, 0.5), torch.full_like(dbk, -0.25)
    ops.linear_bwd_weight(dy, x, into=(acc_w, acc_b))
    assert rel_l2(acc_w - 0.5, dwk) < 1e-5 and rel_l2(acc_b + 0.25, dbk) < 1e-5
    (pre2, pre2d) = _b(_r(rng, M, K))
    p2 = pre2d.clone().requires_grad_(True)
    fac = torch.ones(M, K, dtype=torch.float64)
    if act:
        orc._ACTS[act](p2).backward(torch.ones(M, K, dtype=torch.float64))
        fac = p2.grad
    got = ops.linear_bwd_data(dy, w.to(DEV), pre=pre2 if act else None, act=act)
    assert got.dtype == BF and rel_l2(got, (dyd @ w.double()) * fac) < TOL


@pytest.mark.parametrize("policy", ["force", "off"])
@pytest.mark.parametrize("B,H,W,C", [(2, 64, 64, 256), (1, 21, 17, 128), (2, 16, 16, 32), (1, 12, 20, 192)])
def test_conv_bf16(kernel_env, B, H, W, C, policy):
    """both conv kernels (halo tile in LDS / plain implicit GEMM) with bf16 in, bf16 out; weight gradient straight from
    the bf16 tensors (they ARE the 1-plane operand images), fp32 out"""
    from transformerbasednavierstokesolver_amd import ops
    from oracle import transolver_oracle as orc
    kernel_env(PA2D_CONV_HALO=policy)
    rng = np.random.default_rng(B * H + C)
    N = H * W
    (xn, xnd), (dout, doutd) = _b(_r(rng, B, N, C)), _b(_r(rng, B, N, 2 * C))
    wx, wf = _r(rng, C, C, 3, 3, scale=(9 * C) ** -0.5), _r(rng, C, C, 3, 3, scale=(9 * C) ** -0.5)
    bx, bf = 0.1 * _r(rng, C), 0.1 * _r(rng, C)
    xq = xnd.clone().requires_grad_(True)
    wxd, wfd, bxd, bfd = (t.double().requires_grad_(True) for t in (wx, wf, bx, bf))
    out_o = torch.cat([orc.conv3x3(xq, wxd, bxd, H, W), orc.conv3x3(xq, wfd, bfd, H, W)], -1)
    out_o.backward(doutd)
    g = lambda t: t.to(DEV)
    out = ops.conv3x3x2_fwd(xn, g(wx), g(bx), g(wf), g(bf), H, W)
    assert out.dtype == BF and rel_l2(out, out_o) < TOL
    dxn, dwx, dbx, dwf, dbf = ops.conv3x3x2_bwd(dout, xn, g(wx), g(wf), H, W)
    assert dxn.dtype == BF and dwx.dtype == torch.float32
    assert rel_l2(dxn, xq.grad) < TOL
    assert rel_l2(dwx, wxd.grad) < 1e-4 and rel_l2(dwf, wfd.grad) < 1e-4         # exact bf16 products, fp32 sums
    assert rel_l2(dbx, bxd.grad) < 1e-4 and rel_l2(dbf, bfd.grad) < 1e-4
    into = tuple(torch.full_like(t, 0.125) for t in (dwx, dbx, dwf, dbf))
    ops.conv3x3x2_bwd(dout, xn, g(wx), g(wf), H, W, need_dx=False, into=into)
    for got, ref in zip(into, (dwx, dbx, dwf, dbf)):
        assert rel_l2(got - 0.125, ref) < 1e-5
    # inside a weights_frozen scope the calls run from PRE-MADE packs (narrow shapes included): same results bit for bit
    with ops.weights_frozen():
        for _ in range(2):
            assert torch.equal(ops.conv3x3x2_fwd(xn, g(wx), g(bx), g(wf), g(bf), H, W), out)
            assert torch.equal(ops.conv3x3x2_bwd(dout, xn, g(wx), g(wf), H, W)[0], dxn)


@pytest.mark.parametrize("B,N,heads,D,M", [(2, 30, 4, 8, 12), (2, 4096, 8, 32, 64), (1, 1000, 8, 16, 128),
                                           (1, 1000, 4, 32, 128)])      # last: backward on the exact-fp32 kernel, bf16 storage
def test_slice_path_bf16(B, N, heads, D, M):
    from transformerbasednavierstokesolver_amd import ops
    from oracle import transolver_oracle as orc
    from test_gpu_stages import _slice_inputs
    C = heads * D
    xf32, ws, bs, temp, wq, wk, wv, dy32 = _slice_inputs(B, N, heads, D, M, 3 * B + N + M)
    (xf, xfd), (dy, dyd) = _b(xf32), _b(dy32)
    d = lambda t: t.double()
    w, norm, s, tok = orc.slice_tokens(xfd[..., :C], xfd[..., C:], d(ws), d(bs), d(temp), heads)
    o = orc.token_attention(tok, d(wq), d(wk), d(wv))
    y = orc.deslice(w, o)
    g = lambda t: t.to(DEV).contiguous()
    spart, npart = ops.slice_scatter(xf, 2 * C, 0, xf, 2 * C, C, g(ws), g(bs), g(temp), B, N, heads, D, M)
    assert spart.dtype == torch.float32
    assert rel_l2(spart.sum(1).view(B, heads, M, D), s) < 1e-4 and rel_l2(npart.sum(1).view(B, heads, M), norm) < 1e-4
    of = g(o.float().reshape(B * heads, M, D))
    yk = ops.deslice_fwd(xf, 2 * C, 0, of, g(ws), g(bs), g(temp), B, N, heads, D, M)
    assert yk.dtype == BF and rel_l2(yk, y) < TOL
    ref = orc.slice_core_backward(xfd[..., :C], xfd[..., C:], dyd, d(ws), d(bs), d(temp), d(wq), d(wk), d(wv), heads)
    dopart, _ = ops.slice_scatter(xf, 2 * C, 0, dy, C, 0, g(ws), g(bs), g(temp), B, N, heads, D, M, want_norm=False)
    assert rel_l2(dopart.sum(1).view(B, heads, M, D), ref["do"]) < 1e-4
    f32 = lambda t, *shape: g(t.float().reshape(*shape))
    dxf, dws, dbs, dtemp = ops.slice_bwd_points(xf, dy, g(ws), g(bs), g(temp), of, f32(ref["ds"], B * heads, M, D),
                                                f32(ref["dn"], B * heads, M), B, N, heads, D, M)
    assert dxf.dtype == BF and dws.dtype == torch.float32
    assert rel_l2(dxf[..., :C], ref["dxm"]) < TOL and rel_l2(dxf[..., C:], ref["dfm"]) < TOL
    assert rel_l2(dws, ref["dws"]) < 1e-3 and rel_l2(dbs, ref["dbs"]) < 1e-3
    assert rel_l2(dtemp.reshape(-1), ref["dtemperature"].reshape(-1)) < 1e-3


def test_head_bf16():
    from transformerbasednavierstokesolver_amd import ops
    rng = np.random.default_rng(4)
    (x, xd) = _b(_r(rng, 500, 64))
    w, b, dy = _r(rng, 2, 64), _r(rng, 2), _r(rng, 500, 2)
    y = ops.head_fwd(x, w.to(DEV), b.to(DEV))
    assert y.dtype == torch.float32 and rel_l2(y, xd @ w.double().t() + b.double()) < 1e-5
    dxn, dw, db = ops.head_bwd(dy.to(DEV), x, w.to(DEV))
    assert dxn.dtype == BF and rel_l2(dxn, dy.double() @ w.double()) < TOL
    assert rel_l2(dw, dy.double().t() @ xd) < 1e-5 and rel_l2(db, dy.double().sum(0)) < 1e-5


def test_full_ns_model_bf16_storage_forward_and_backward():
    """BASELINE configs[2] numerics on the configs[1] architecture (8 layers, C=256, M=64): forward vs the reference-made
    fp64 fixture G5 <= 3e-2, and really in reduced precision (> 1e-4); gradients finite and within 0.2 of
    the fp64 ones in norm (bf16 autocast-level agreement)."""
    from transformerbasednavierstokesolver_amd import synth, harness, ops
    from transformerbasednavierstokesolver_amd.utils.testloss import TestLoss
    g = np.load(os.path.join(GOLDEN, "G5_full_ns.npz"))
    cfg = synth.NS_CONFIG
    m = harness.build_model(cfg, synth.synth_state_dict(cfg, seed=51), DEV, engine="bf16s")
    assert harness.model_engine(m) == ops.ENGINE_BF16S
    pos, a, u = synth.ns_batch(1, seed=52)
    x, fx, y = (torch.from_numpy(t).to(DEV) for t in (pos, a, u[..., :1]))
    pred = m(x, fx=fx)
    assert pred.dtype == torch.float32
    e = rel_l2(pred.reshape(-1), g["pred"])
    assert 1e-4 < e < 3e-2, e
    loss = TestLoss(size_average=False)(pred.reshape(1, -1), y.reshape(1, -1))
    assert abs(loss.item() - float(g["loss"])) < 3e-2 * float(g["loss"])
    loss.backward()
    for k, p in m.named_parameters():
        if k == "placeholder":
            continue
        assert p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all(), k
        n, ref = float(p.grad.double().norm()), float(g["grad.norm." + k])
        if "to_q" in k or "to_k" in k:          # near-uniform attention at init: tiny, noise-dominated gradients
            continue
        assert abs(n - ref) < 0.2 * ref, (k, n, ref)


def test_training_trajectory_bf16_storage_tracks_the_fp64_oracle():
    """4 exp_ns-style iterations (FusedAdamW on fp32 master weights, fp32 gradient bucket fed by bf16-storage kernels)
    vs the fp64 oracle trained by torch AdamW on the same data: the loss tracks within 5 % at every step."""
    from transformerbasednavierstokesolver_amd import synth, harness
    from transformerbasednavierstokesolver_amd.optim import FusedAdamW
    from transformerbasednavierstokesolver_amd.utils.testloss import FusedTestLoss
    from oracle import transolver_oracle as orc
    cfg = dict(synth.NS_SMALL_CONFIG, n_layers=2, H=16, W=16)
    sd = synth.synth_state_dict(cfg, seed=131)
    m = harness.build_model(cfg, sd, DEV, engine="bf16s").train()
    pos, a, u = synth.ns_batch(3, 16, 16, seed=132)
    x, fx, yy = (torch.from_numpy(t) for t in (pos, a, u[..., :3]))
    opt = FusedAdamW(m.parameters(), lr=2e-3, weight_decay=1e-5, max_grad_norm=0.5)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=2e-3, total_steps=10)
    sdo = orc.to_torch(sd, torch.float64, requires_grad=True)
    live = [k for k in sdo if k != "placeholder"]
    oo = torch.optim.AdamW([sdo[k] for k in live], lr=2e-3, weight_decay=1e-5)
    so = torch.optim.lr_scheduler.OneCycleLR(oo, max_lr=2e-3, total_steps=10)
    for it in range(4):
        loss, _ = harness.train_step(m, opt, sched, x.to(DEV), fx.to(DEV), yy.to(DEV), grad_sync=opt.sync,
                                     loss_fn=FusedTestLoss(size_average=False))
        oo.zero_grad()
        lo, _, _, grads = orc.train_iteration(sdo, x.double(), fx.double(), yy.double(), cfg)
        for k in live:
            sdo[k].grad = grads[k]
        torch.nn.utils.clip_grad_norm_([sdo[k] for k in live], 0.5)
        oo.step()
        so.step()
        assert abs(loss.item() - lo.item()) < 5e-2 * abs(lo.item()), (it, loss.item(), lo.item())
    assert all(p.dtype == torch.float32 for p in m.parameters())                 # fp32 master weights


def test_darcy_421_block_bf16_storage():
    """BASELINE configs[4] geometry in its stated numerics: one Physics-Attention block at 421 x 421, C=128, M=128 fed
    bf16, against the fp64 oracle on the GPU evaluated on the same bf16 values."""
    from test_gpu_darcy import conv3x3_shifted
    from transformerbasednavierstokesolver_amd import synth
    from transformerbasednavierstokesolver_amd.model.Physics_Attention import Physics_Attention_Structured_Mesh_2D
    from oracle import transolver_oracle as orc
    H = W = 421
    C, h, M = 128, 8, 128
    cfg = synth.make_config(n_layers=1, n_hidden=C, n_head=h, slice_num=M, fun_dim=1, H=H, W=W)
    pre = "blocks.0.Attn."
    sd = {k[len(pre):]: torch.from_numpy(v) for k, v in synth.synth_state_dict(cfg, seed=71).items() if k.startswith(pre)}
    a = Physics_Attention_Structured_Mesh_2D(C, heads=h, dim_head=C // h, slice_num=M, H=H, W=W)
    a.load_state_dict(sd, strict=True)
    a = a.to(DEV)
    g = torch.Generator(device=DEV).manual_seed(72)
    x = torch.randn(1, H * W, C, device=DEV, generator=g).to(BF).requires_grad_(True)
    gy = torch.randn(1, H * W, C, device=DEV, generator=g).to(BF)
    y = a(x)
    assert y.dtype == BF
    y.backward(gy)
    sdo = {pre + k: v.to(DEV).double().requires_grad_(True) for k, v in sd.items()}
    xo = x.detach().double().requires_grad_(True)
    real = orc.conv3x3
    orc.conv3x3 = conv3x3_shifted
    try:
        yo = orc.physics_attention(xo, sdo, pre, H, W, h)
        yo.backward(gy.double())
    finally:
        orc.conv3x3 = real
    assert rel_l2(y, yo) < 3e-2
    assert rel_l2(x.grad, xo.grad) < 5e-2
    for k, p in a.named_parameters():
        if "to_q" in k or "to_k" in k:
            continue
        assert rel_l2(p.grad, sdo[pre + k].grad) < 5e-2, k
