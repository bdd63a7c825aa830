"""The fused block tail (ops.block_tail_fwd, csrc/pa2d_block_tail.hip) on the GPU.

Stages, per element.  One call with the three debug outputs inside `poisoned(...)`, against an fp64 restatement in plain
torch; bounds are the suite's own (tests/elementwise_check.py) for the split engine, the only engine the kernel has:
  y, h, xn     check_rows at ROW_TOL["split"] against the fp64 chain (every stage from the fp64 value of the one before);
  a, h, out    check_products at TAU[("split", "fwd")], scale = the same stage on absolute values, judged ALONE: the operand
               is the previous stage's value as the kernel produced it (its debug output), taken to fp64, so an error of an
               earlier stage is not charged to a later one and cannot hide in its scale.  The same ratio against the fp64
               chain is printed, not asserted: there the rounding of `a` (bounded by |y| |Wo|^T + |fx|) is charged to
               `out`, whose scale |h| |W2|^T + |a| knows nothing of it — where a row of `a` cancels (tokens 1e3 apart per
               sample) that figure is 3e-4 with every stage exact to 2e-7 on its own.
Shapes: R = 3 x 77 = 231 rows (odd, a partial last panel, and a sample boundary inside a panel for both panel heights; N = 77
is no multiple of 16), R = one panel and one panel + 1 for both panel heights, a residual stream 100 x the branch, and
tokens whose scale differs by sample by 1e3 per sample (a panel that reads the neighbour's tokens is off by that factor).

MI355X, worst figure over every case of this file (bound): y rows 1.8e-6 (9e-6: heads 8, D 16, M 128), h rows 9.2e-7,
xn rows 1.0e-6; per element, stage alone: a 2.7e-7, h 2.7e-7, out 2.2e-7 of the scale (1.6e-6).  Both panel heights give the
same figures (rows are independent).  Models, fused / unfused rel-L2 against fp64 and their ratio: 2-D 1.56e-7 / 1.52e-7 =
1.03, irregular 1.77e-7 / 1.67e-7 = 1.06, 3-D 3.00e-7 / 3.02e-7 = 0.99; 3-step rollout 6.96e-7 / 7.57e-7 = 0.92.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from elementwise_check import ROW_TOL, TAU, check_products, check_rows, poisoned

pytestmark = pytest.mark.gpu
DEV = "cuda"
ENGINE = "split"
TEMPS = np.array([0.03, 0.5, 7.0, 0.25, 1.5, 0.1, 5.0, 0.8], dtype=np.float32)      # clamp active at both ends
TEMPS_RAW = np.array([0.4, 0.5, 1.3, 0.25], dtype=np.float32)                        # irregular mesh: used as they are


def _acts():
    sp = lambda z: torch.where(z > 20, z, torch.log1p(torch.exp(z.clamp(max=20))))
    return {"gelu": lambda z: 0.5 * z * (1 + torch.erf(z * 2 ** -0.5)), "tanh": torch.tanh, "sigmoid": torch.sigmoid,
            "relu": torch.relu, "softplus": sp, "ELU": F.elu, "silu": F.silu, None: lambda z: z}


def _ln(x, g, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-5) * g + b


def _inputs(B, N, heads, D, M, r, clamp, seed, fx_scale=1.0, o_by_sample=1.0):
    g = torch.Generator().manual_seed(seed)
    C, hid = heads * D, r * heads * D
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(DEV)
    t = dict(xf=rn(B, N, 2 * C), o=rn(B * heads, M, D), ws=rn(M, D, scale=D ** -0.5), bs=rn(M, scale=0.3),
             temp=torch.tensor(np.resize(TEMPS if clamp else TEMPS_RAW, heads)).to(DEV),
             fx=rn(B * N, C, scale=fx_scale), wo=rn(C, C, scale=C ** -0.5), bo=rn(C, scale=0.1),
             g2=1 + rn(C, scale=0.1), be2=rn(C, scale=0.1), w1=rn(hid, C, scale=C ** -0.5), b1=rn(hid, scale=0.1),
             w2=rn(C, hid, scale=hid ** -0.5), b2=rn(C, scale=0.1), gn=1 + rn(C, scale=0.1), bn=rn(C, scale=0.1))
    if o_by_sample != 1.0:
        t["o"] = (t["o"].view(B, heads, M, D) * (o_by_sample ** torch.arange(B, device=DEV).float()).view(B, 1, 1, 1)).reshape(
            B * heads, M, D).contiguous()
    return t


def _reference(t, B, N, heads, D, M, act, clamp, got):
    """fp64: the chain (each stage from the fp64 value of the one before) and, for the product stages, the stage ALONE
    from the kernel's own previous output `got` = (y, a, h, out) with its absolute-value scale."""
    d = {k: v.double() for k, v in t.items()}
    C = heads * D
    f = _acts()[act]
    xm = d["xf"][..., :C].reshape(B, N, heads, D).permute(0, 2, 1, 3)
    tau = d["temp"].reshape(1, heads, 1, 1)
    tau = tau.clamp(0.1, 5.0) if clamp else tau
    w = torch.softmax((xm @ d["ws"].t() + d["bs"]) / tau, -1)
    y = (w @ d["o"].view(B, heads, M, D)).permute(0, 2, 1, 3).reshape(B * N, C)
    lin = lambda x, wt, b: x @ wt.t() + b
    a = lin(y, d["wo"], d["bo"]) + d["fx"]
    h = f(lin(_ln(a, d["g2"], d["be2"]), d["w1"], d["b1"]))
    out = lin(h, d["w2"], d["b2"]) + a
    chain = dict(y=y, a=a, h=h, out=out, xn=_ln(out, d["gn"], d["bn"]))
    yk, ak, hk, _ = (g.double() for g in got)
    alone, scale = {}, {}
    for tag, yo, ao, ho in (("alone", yk, ak, hk), ("chain", y, a, h)):
        xn2 = _ln(ao, d["g2"], d["be2"])
        alone[tag] = dict(a=lin(yo, d["wo"], d["bo"]) + d["fx"], h=f(lin(xn2, d["w1"], d["b1"])), out=lin(ho, d["w2"], d["b2"]) + ao)
        scale[tag] = dict(a=lin(yo.abs(), d["wo"].abs(), d["bo"].abs()) + d["fx"].abs(),
                          h=lin(xn2.abs(), d["w1"].abs(), d["b1"].abs()),
                          out=lin(ho.abs(), d["w2"].abs(), d["b2"].abs()) + ao.abs())
    return chain, alone, scale


def _run_stage_case(B, N, heads, D, M, r, act="gelu", clamp=True, seed=0, trailing=True, **kw):
    from transformerbasednavierstokesolver_amd import ops
    C = heads * D
    t = _inputs(B, N, heads, D, M, r, clamp, seed, **kw)
    gn, bn = (t["gn"], t["bn"]) if trailing else (None, None)
    assert ops.block_tail_supported(C, heads, D, M, r * C, act, ENGINE)
    call = lambda: ops.block_tail_fwd(t["xf"], 2 * C, 0, t["o"], t["ws"], t["bs"], t["temp"], t["fx"], t["wo"], t["bo"],
                                      t["g2"], t["be2"], t["w1"], t["b1"], t["w2"], t["b2"], gn, bn, B, N, heads, D, M, act,
                                      clamp=clamp, engine=ENGINE, debug=True)
    out, xn, (y, a, h) = poisoned(call)
    assert (xn is None) == (not trailing)
    chain, alone, scale = _reference(t, B, N, heads, D, M, act, clamp, (y, a, h, out))
    tag = f"tail B={B} N={N} heads={heads} D={D} M={M} r={r} act={act} clamp={clamp} {kw}"
    rt, tau = ROW_TOL[ENGINE], TAU[(ENGINE, "fwd")]
    fig = dict(y=check_rows(y, chain["y"], float("inf")), h_rows=check_rows(h, chain["h"], float("inf")))
    if trailing:
        fig["xn"] = check_rows(xn, chain["xn"], float("inf"))
    for k, gotk in (("a", a), ("h", h), ("out", out)):
        for ref in ("alone", "chain"):
            fig[f"{k}_{ref}"] = check_products(gotk, alone[ref][k], scale[ref][k], float("inf"))
    print(f"{tag}: " + ", ".join(f"{k} {v:.3g}" for k, v in fig.items()))      # every figure before any assertion
    check_rows(y, chain["y"], rt, label=tag + " y [row, c]")
    check_rows(h, chain["h"], rt, label=tag + " h [row, hidden]")
    if trailing:
        check_rows(xn, chain["xn"], rt, label=tag + " xn [row, c]")
    for k, gotk in (("a", a), ("h", h), ("out", out)):
        check_products(gotk, alone["alone"][k], scale["alone"][k], tau, label=f"{tag} {k} [row, col]")
    # without the debug outputs and inside a frozen scope (ready-made images): the same bits
    with ops.weights_frozen():
        out2, xn2, dbg = ops.block_tail_fwd(t["xf"], 2 * C, 0, t["o"], t["ws"], t["bs"], t["temp"], t["fx"], t["wo"], t["bo"],
                                            t["g2"], t["be2"], t["w1"], t["b1"], t["w2"], t["b2"], gn, bn, B, N, heads, D, M,
                                            act, clamp=clamp, engine=ENGINE)
    assert dbg is None and torch.equal(out2, out) and (xn is None or torch.equal(xn2, xn))
    return fig


STAGE_SHAPES = [  # heads, D, M, r, clamp
    (8, 32, 64, 1, True),        # NS / bench
    (8, 16, 64, 2, True),        # pipe
    (8, 8, 32, 4, True),
    (8, 16, 128, 1, True),
    (4, 16, 12, 1, False),       # irregular mesh: raw temperature
]


@pytest.mark.parametrize("panel", ["16", "32"])
@pytest.mark.parametrize("heads,D,M,r,clamp", STAGE_SHAPES)
def test_stages(kernel_env, heads, D, M, r, clamp, panel):
    """B = 3, N = 77 (R = 231) at both panel heights.  MI355X, worst over these cases: y 1.8e-6, h rows 8.9e-7, xn 7.5e-7
    (9e-6); a 2.7e-7, h 2.7e-7, out 2.1e-7 of the scale (1.6e-6)."""
    kernel_env(PA2D_TAIL_PANEL=panel)
    _run_stage_case(3, 77, heads, D, M, r, clamp=clamp, seed=heads + D + M + r)


@pytest.mark.parametrize("panel,R", [("16", 16), ("16", 17), ("32", 32), ("32", 33), (None, 1)])
def test_one_panel_and_one_more(kernel_env, panel, R):
    kernel_env(PA2D_TAIL_PANEL=panel)
    _run_stage_case(1, R, 8, 16, 64, 2, seed=R)
    _run_stage_case(1, R, 8, 16, 64, 2, seed=R, trailing=False)


@pytest.mark.parametrize("panel", ["16", "32"])
def test_strong_residual_and_tokens_that_differ_by_sample(kernel_env, panel):
    kernel_env(PA2D_TAIL_PANEL=panel)
    _run_stage_case(3, 77, 8, 16, 64, 2, seed=5, fx_scale=100.0)
    # N = 5: up to four (P = 16) / seven (P = 32) samples inside one panel, tokens 1e3 apart from sample to sample
    _run_stage_case(7, 5, 8, 16, 64, 2, seed=6, o_by_sample=1e3)
    _run_stage_case(3, 77, 4, 16, 12, 1, clamp=False, seed=7, o_by_sample=1e-3)


@pytest.mark.parametrize("act", ["tanh", "sigmoid", "relu", "softplus", "ELU", "silu", None])
def test_every_activation(act):
    _run_stage_case(3, 77, 8, 8, 32, 4, act=act, seed=11)


# ---------------------------------------------------------------------------------------------- models
def _forward3d_f64(sd, x, fx, H, W, Dd, heads):
    """fp64 statement of the 3-D structured model from the oracle's pieces (the oracle has the 2-D and the irregular model)."""
    from oracle import transolver_oracle as orc
    z = orc.mlp(torch.cat((x, fx), -1), sd, "preprocess.")
    L = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    B, N, C = z.shape

    def conv(xn, w, b):
        img = xn.reshape(B, H, W, Dd, C).permute(0, 4, 1, 2, 3)
        return F.conv3d(img, w, b, padding=1).permute(0, 2, 3, 4, 1).reshape(B, N, C)

    for i in range(L):
        p = f"blocks.{i}."
        a = p + "Attn."
        xn = orc.layer_norm(z, sd[p + "ln_1.weight"], sd[p + "ln_1.bias"])
        xm, fm = conv(xn, sd[a + "in_project_x.weight"], sd[a + "in_project_x.bias"]), conv(
            xn, sd[a + "in_project_fx.weight"], sd[a + "in_project_fx.bias"])
        w, _, _, tok = orc.slice_tokens(xm, fm, sd[a + "in_project_slice.weight"], sd[a + "in_project_slice.bias"],
                                        sd[a + "temperature"], heads)
        o = orc.token_attention(tok, sd[a + "to_q.weight"], sd[a + "to_k.weight"], sd[a + "to_v.weight"])
        z = orc.deslice(w, o) @ sd[a + "to_out.0.weight"].t() + sd[a + "to_out.0.bias"] + z
        z = orc.mlp(orc.layer_norm(z, sd[p + "ln_2.weight"], sd[p + "ln_2.bias"]), sd, p + "mlp.") + z
    p = f"blocks.{L - 1}."
    return orc.layer_norm(z, sd[p + "ln_3.weight"], sd[p + "ln_3.bias"]) @ sd[p + "mlp2.weight"].t() + sd[p + "mlp2.bias"]


def _tiny(kind, mlp_ratio=2):
    from transformerbasednavierstokesolver_amd.model import Transolver_Irregular_Mesh as irregular
    from transformerbasednavierstokesolver_amd.model import Transolver_Structured_Mesh_2D as structured
    from transformerbasednavierstokesolver_amd.model import Transolver_Structured_Mesh_3D as structured3d
    torch.manual_seed(3)
    kw = dict(n_layers=2, n_hidden=64, n_head=4, fun_dim=3, out_dim=1, slice_num=8, mlp_ratio=mlp_ratio)
    if kind == "2d":
        m, N, sdim = structured.Model(space_dim=2, H=5, W=7, **kw), 35, 2
    elif kind == "irregular":
        m, N, sdim = irregular.Model(space_dim=2, **kw), 33, 2
    else:
        m, N, sdim = structured3d.Model(space_dim=3, H=2, W=3, D=4, **kw), 24, 3
    with torch.no_grad():      # the default init leaves biases 0 and LayerNorms at identity: move them
        for k, p in m.named_parameters():
            if k.endswith("bias") or ".ln_" in k:
                p.add_(0.1 * torch.randn_like(p))
    g = torch.Generator().manual_seed(4)
    x, fx = torch.rand(3, N, sdim, generator=g), torch.randn(3, N, 3, generator=g)
    return m.to(DEV).eval().set_engine(ENGINE), x.to(DEV), fx.to(DEV), N


def _spy(monkeypatch, names):
    from transformerbasednavierstokesolver_amd import ops
    calls = []
    for name in names:
        def spy(*a, _f=getattr(ops, name), _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, spy)
    return calls


def _row_rel(got, ref):
    return check_rows(got.reshape(got.shape[0], -1), ref.reshape(ref.shape[0], -1), float("inf"))


@pytest.mark.parametrize("kind", ["2d", "irregular", "3d"])
def test_models_against_unfused_and_fp64(monkeypatch, kind):
    """Fused forward, unfused forward and the fp64 oracle on the same inputs (tiny models, B = 3): the fused path's max
    per-sample rel-L2 against fp64 is <= max(ROW_TOL, 4 x the unfused path's own), the rule of test_gpu_darcy_loss.py.
    The model's output has one channel, so a row is a sample's field.  MI355X: ratios 1.03 (2-D), 1.06 (irregular),
    0.99 (3-D); both paths at 1.5e-7 .. 3.0e-7, far below the floor."""
    from oracle import transolver_oracle as orc
    model, x, fx, N = _tiny(kind)
    conv = {"2d": "conv3x3x2_fwd", "irregular": "linear_fwd", "3d": "conv3x3x3x2_fwd"}[kind]
    calls = _spy(monkeypatch, ["layernorm_fwd", "layernorm_fwd_planes", "conv3x3x2_fwd", "conv3x3x2_fwd_planes",
                               "conv3x3x3x2_fwd", "linear_fwd", "slice_scatter", "token_attn_fwd", "deslice_fwd",
                               "block_tail_fwd", "head_fwd"])
    with torch.no_grad():
        base = model(x, fx=fx)
        assert "block_tail_fwd" not in calls and calls.count("deslice_fwd") == 2
        del calls[:]
        fused = model.set_fused_tail(True)(x, fx=fx)
    want = ["linear_fwd"] * 2 + ["layernorm_fwd"] + [conv, "slice_scatter", "token_attn_fwd", "block_tail_fwd"] * 2 + ["head_fwd"]
    assert calls == want, calls                      # four calls per block, ln_1 once, the head last
    sd = orc.to_torch({k: v.detach().cpu() for k, v in model.state_dict().items()}, torch.float64)
    xd, fd = x.double().cpu(), fx.double().cpu()
    if kind == "2d":
        ref = orc.model_forward(sd, xd, fd, dict(H=5, W=7, ref=8, unified_pos=False, n_head=4))
    elif kind == "irregular":
        ref = orc.model_forward_irregular(sd, xd, fd, dict(ref=8, unified_pos=False, n_head=4))
    else:
        ref = _forward3d_f64(sd, xd, fd, 2, 3, 4, 4)
    e_fused, e_base = _row_rel(fused.cpu(), ref), _row_rel(base.cpu(), ref)
    print(f"{kind}: fused vs fp64 {e_fused:.3g}, unfused vs fp64 {e_base:.3g}, ratio {e_fused / max(e_base, 1e-300):.3g}")
    assert e_fused <= max(ROW_TOL[ENGINE], 4 * e_base), (e_fused, e_base)


@pytest.mark.parametrize("how", ["train", "grad", "bf16s", "generic_mlp"])
def test_fallbacks_are_todays_bits(how):
    model, x, fx, N = _tiny("2d")
    if how == "generic_mlp":
        torch.manual_seed(9)
        for b in model.blocks:
            b.mlp.linears.append(torch.nn.Sequential(torch.nn.Linear(b.mlp.n_hidden, b.mlp.n_hidden), torch.nn.GELU()).to(DEV))
            b.mlp.n_layers = 1
    if how == "bf16s":
        model.set_engine("bf16s")
    if how == "train":
        model.train()
    ctx = torch.enable_grad if how == "grad" else torch.no_grad
    with ctx():
        base = model.set_fused_tail(False)(x, fx=fx).detach().clone()
        flagged = model.set_fused_tail(True)(x, fx=fx).detach()
    assert torch.equal(flagged, base)


# ---------------------------------------------------------------------------------------------- rollout
def test_rollout_eager_graphed_and_refresh():
    from transformerbasednavierstokesolver_amd import harness
    from transformerbasednavierstokesolver_amd.model import Transolver_Structured_Mesh_2D as structured
    torch.manual_seed(1)
    model = structured.Model(space_dim=2, n_layers=2, n_hidden=64, n_head=4, fun_dim=4, out_dim=1, slice_num=16, mlp_ratio=2,
                             H=16, W=16).to(DEV).eval().set_engine(ENGINE)
    g = torch.Generator().manual_seed(2)
    x, fx = torch.rand(2, 256, 2, generator=g).to(DEV), torch.randn(2, 256, 4, generator=g).to(DEV)
    base = harness.rollout(model, x, fx, 3)
    eager = harness.rollout(model, x, fx, 3, fused_tail=True)
    assert model.fused_tail is False and not any(b.fused_tail for b in model.blocks)
    gr = harness.GraphedRollout(model, x, fx, fused_tail=True)
    assert model.fused_tail is False and not any(b.fused_tail for b in model.blocks)
    graphed = gr.run(fx, 3)
    assert torch.equal(graphed, eager)
    # against the unfused rollout, by the rule of the model test: both against the fp64 oracle's rollout, rows = the
    # (sample, frame) fields
    from oracle import transolver_oracle as orc
    sd = orc.to_torch({k: v.detach().cpu() for k, v in model.state_dict().items()}, torch.float64)
    ref = orc.rollout(sd, x.double().cpu(), fx.double().cpu(), dict(H=16, W=16, ref=8, unified_pos=False, n_head=4), 3)
    rows = lambda t: t.detach().cpu().permute(0, 2, 1)
    e_fused, e_base = check_rows(rows(eager), rows(ref), float("inf")), check_rows(rows(base), rows(ref), float("inf"))
    print(f"rollout: fused vs fp64 {e_fused:.3g}, unfused vs fp64 {e_base:.3g}")
    assert e_fused <= max(ROW_TOL[ENGINE], 4 * e_base), (e_fused, e_base)
    assert torch.equal(harness.rollout(model, x, fx, 3), base)                  # and the default route is untouched
    with torch.no_grad():      # weights moved in place: run() must refresh the tail's images
        for b in model.blocks:
            b.Attn.to_out[0].weight.mul_(1.5)
            b.mlp.linear_pre[0].weight.add_(0.01)
            b.ln_2.weight.mul_(0.9)
    again = gr.run(fx, 3)
    fresh = harness.rollout(model, x, fx, 3, fused_tail=True)
    assert torch.equal(again, fresh) and not torch.equal(again, graphed)
