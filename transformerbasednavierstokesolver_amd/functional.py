"""Forward/backward compositions of the libpa2d stages and their autograd wrappers.

One autograd node per stage group (LayerNorm, Physics-Attention incl. to_out + residual, MLP incl.
residual, head) instead of the ~120 nodes per layer the reference builds; the slice
weights [B,h,N,M] are never saved — backward recomputes them from x_mid inside the kernels.
"""
from __future__ import annotations

import torch
from torch.autograd import Function

from . import ops


# ------------------------------------------------------------------------------ direct gradient accumulation
def grad_targets(params):
    """Flat-bucket gradient views of `params` if EVERY one of them is managed by a gradient bucket
    (ddp.FlatGradSync, which tags its parameters with `_pa2d_slot`), else None.  With targets the backward
    kernels add their result straight into the bucket (`accumulate = 1`) and the autograd node returns None for
    those parameters — no per-call gradient tensors, no torch `add_` launches, no copies."""
    slots = [getattr(p, "_pa2d_slot", None) for p in params]
    if not slots or any(s is None for s in slots):
        return None
    return tuple(sync.target(i) for sync, i in slots)


def _ret(targets, grads):
    """Gradients to hand back to autograd: None for everything that was accumulated in place."""
    return tuple(None for _ in grads) if targets is not None else tuple(grads)


# ------------------------------------------------------------------------------ Physics-Attention
def mesh_extent(W):
    """(width, depth) of a structured mesh: the geometry argument `W` of the functions below is the width of a 2-D mesh
    (depth None: 3x3 conv projections) or the pair (width, depth) of a 3-D mesh [H, W, depth] (3x3x3 conv projections,
    Physics_Attention_Structured_Mesh_3D)."""
    return (W[0], W[1]) if isinstance(W, tuple) else (W, None)


def dropout_draws(p, B, N, C, heads, M):
    """The two draws of one Physics-Attention layer in training mode with dropout p > 0, reserved from the package
    generator IN THIS ORDER: the attention matrix (B*heads*M*M elements, Physics_Attention.py:110), then the output of
    to_out (B*N*C, :28).  Each is the `drop` tuple (thresh, scale, seed, offset) of the ops.  Blocks reserve in model order."""
    ts = ops.dropout_constants(p)
    return ts + ops.dropout_reserve(B * heads * M * M), ts + ops.dropout_reserve(B * N * C)


def project_fwd(xn, P, geom, engine, xn_planes=None, shape=None):
    """[x_mid | fx_mid] [B,N,2C] of xn [B,N,C] on the geometry geom = (H, W) of attn_forward: the 3x3 conv pair, the 3x3x3
    pair of a 3-D mesh (W = (width, depth)), the pair on the operand planes `xn_planes` (xn is then None and shape =
    (B, N, C)), or, H None, the two Linear(C, C) of the irregular mesh as ONE GEMM with the weights stacked along the output
    dim.  Returns (xf, kept); kept = (the operand, the stacked weight or None, (B, N, C)) is what project_bwd takes."""
    H, W = geom
    B, N, C = shape = tuple(xn.shape) if xn is not None else shape
    Wm, depth = mesh_extent(W)
    wcat = None
    if xn_planes is not None:
        if depth is not None:
            raise ValueError("the operand-planes route is 3x3 only; the 3-D mesh takes the fp32 operand")
        xf = ops.conv3x3x2_fwd_planes(xn_planes, P["wx"], P["bx"], P["wf"], P["bf"], B, H, W, engine)
    elif H is not None and depth is not None:
        xf = ops.conv3x3x3x2_fwd(xn, P["wx"], P["bx"], P["wf"], P["bf"], H, Wm, depth, engine=engine)
    elif H is not None:
        xf = ops.conv3x3x2_fwd(xn, P["wx"], P["bx"], P["wf"], P["bf"], H, W, engine=engine)
    else:   # the stacked weight is a temporary: a weights_frozen() scope gets no entry for it
        wcat, bcat = torch.cat((P["wx"], P["wf"]), 0), torch.cat((P["bx"], P["bf"]), 0)
        with ops.unscoped():
            xf = ops.linear_fwd(xn.view(B * N, C), wcat, bcat, engine=engine)[0].view(B, N, 2 * C)
    return xf, (xn if xn_planes is None else xn_planes, wcat, shape)


def project_bwd(dxf, kept, P, geom, engine, need_dx, into, planes):
    """Backward of project_fwd from dxf = [dX | dF] [B,N,2C] (`planes`: its plane image, beside the operand's).  `into`:
    (dwx, dbx, dwf, dbf) buffers to add into, or None.  Returns (dxn or None, the gradients made here as a dict: wx, bx, wf,
    bf; on the planes route wx and wf, the bias gradients come with the slice backward)."""
    H, W = geom
    xn, wcat, (B, N, C) = kept
    Wm, depth = mesh_extent(W)
    if planes:
        dxn, dwx, dwf = ops.conv3x3x2_bwd_planes(dxf, xn, P["wx"], P["wf"], B, H, W, engine, need_dx=need_dx,
                                                 into=None if into is None else (into[0], into[2]))
        return dxn, dict(wx=dwx, wf=dwf)
    if H is not None and depth is not None:
        dxn, dwx, dbx, dwf, dbf = ops.conv3x3x3x2_bwd(dxf, xn, P["wx"], P["wf"], H, Wm, depth, need_dx=need_dx,
                                                      engine=engine, into=into)
    elif H is not None:
        dxn, dwx, dbx, dwf, dbf = ops.conv3x3x2_bwd(dxf, xn, P["wx"], P["wf"], H, W, need_dx=need_dx, engine=engine,
                                                    into=into)
    else:
        dxf2 = dxf.view(B * N, 2 * C)
        dwcat, dbcat = ops.linear_bwd_weight(dxf2, xn.view(B * N, C), engine=engine)
        dwx, dwf, dbx, dbf = dwcat[:C].contiguous(), dwcat[C:].contiguous(), dbcat[:C].contiguous(), dbcat[C:].contiguous()
        dxn = None
        if need_dx:
            with ops.unscoped():
                dxn = ops.linear_bwd_data(dxf2, wcat, engine=engine).view(B, N, C)
    return dxn, dict(wx=dwx, bx=dbx, wf=dwf, bf=dbf)


def _front(xn, P, geom, heads, engine, xn_planes=None, shape=None, drop=None):
    """The front half of a Physics-Attention layer: projection, slice scatter, token attention (`drop`: the draw of the
    attention matrix).  Returns (xf, kept, s, nrm, o, temp): kept as of project_fwd; s, nrm, o the slice tokens, their norms
    and the attended tokens; temp the temperature as the kernels take it.  H None: no temperature clamp."""
    xf, kept = project_fwd(xn, P, geom, engine, xn_planes=xn_planes, shape=shape)
    B, N, C = kept[2]
    D, M = C // heads, P["ws"].shape[0]
    temp = P["temperature"].reshape(heads).contiguous()
    spart, npart = ops.slice_scatter(xf, 2 * C, 0, xf, 2 * C, C, P["ws"], P["bs"], temp, B, N, heads, D, M,
                                     clamp=geom[0] is not None, engine=engine)
    s, nrm, o = ops.token_attn_fwd(spart, npart, P["wq"], P["wk"], P["wv"], **({} if drop is None else dict(drop=drop)))
    return xf, kept, s, nrm, o, temp


def _target_lookup(targets):
    """t(*keys): the gradient buffers of `targets` (dict key -> buffer) under those keys, as the `into` of a backward op;
    None without targets (the op then makes fresh tensors)."""
    if targets is None:
        return lambda *ks: None
    return lambda *ks: tuple(targets[k] for k in ks)


def attn_forward(xn, P, res, H, W, heads, engine=None, xn_planes=None, shape=None, drop=None):
    """xn [B,N,C] (already layer-normed).  P: dict of parameter tensors.  Returns (out, saved).
    H is None -> irregular-mesh variant (Physics_Attention.py:6-57): Linear projections, no
    temperature clamp; otherwise the structured-mesh variant (3x3 conv projections, clamp; W = (width, depth):
    the 3-D structured mesh, 3x3x3 conv projections, clamp).
    xn_planes (structured, bf16 engines): the LayerNorm output exists only as the conv's bf16 plane image
    (ops.layernorm_fwd_planes); `xn` is then None and `shape` = (B, N, C).
    drop: `dropout_draws(...)` — the attention matrix is dropped inside the token kernel, and to_out runs WITHOUT the fused
    residual so that out = res + dropout(to_out(y)) (one flat launch, ops.dropout_residual)."""
    xf, kept, s, nrm, o, temp = _front(xn, P, (H, W), heads, engine, xn_planes, shape, None if drop is None else drop[0])
    B, N, C = kept[2]
    y = ops.deslice_fwd(xf, 2 * C, 0, o, P["ws"], P["bs"], temp, B, N, heads, C // heads, P["ws"].shape[0],
                        clamp=H is not None, engine=engine)                                    # [B,N,C]
    res2d = None if res is None else res.reshape(B * N, C)
    if drop is None:
        out, _ = ops.linear_fwd(y.view(B * N, C), P["wo"], P["bo"], res=res2d, engine=engine)
    else:
        z, _ = ops.linear_fwd(y.view(B * N, C), P["wo"], P["bo"], engine=engine)
        out = ops.dropout_residual(z, res2d, drop[1])
    return out.view(B, N, C), (kept, xf, s, nrm, o, y, temp)


def attn_backward(saved, P, dout, H, W, heads, need_dx=True, engine=None, targets=None, planes=False, drop=None):
    """`targets`: dict ATTN_KEYS -> gradient buffer to ADD into (structured meshes), or None (fresh tensors).
    `planes`: the saved operand is the plane image of the LayerNorm output; the slice backward then emits [dX | dF] as planes
    too (plus the conv bias gradients) and the conv backward consumes both images directly.
    `drop`: the forward's draws; the gradient entering to_out is dout with the output mask made again (the caller keeps
    the undropped dout as the residual gradient).
    Returns (dxn, dict ATTN_KEYS -> gradient); the dict is None where the gradients went into `targets`."""
    kept, xf, s, nrm, o, y, temp = saved
    B, N, C = kept[2]
    D = C // heads
    M = P["ws"].shape[0]
    d2 = dout.reshape(B * N, C)
    if drop is not None:
        d2 = ops.dropout_residual(d2, None, drop[1])
    structured = H is not None
    if planes and mesh_extent(W)[1] is not None:
        raise ValueError("the operand-planes route is 3x3 only; the 3-D mesh takes the fp32 operand")
    T = targets if structured else None
    t = _target_lookup(T)
    dy = ops.linear_bwd_data(d2, P["wo"], engine=engine)                                      # [B*N,C]
    dwo, dbo = ops.linear_bwd_weight(d2, y.view(B * N, C), engine=engine, into=t("wo", "bo"))
    dopart, _ = ops.slice_scatter(xf, 2 * C, 0, dy, C, 0, P["ws"], P["bs"], temp, B, N, heads, D, M,
                                  want_norm=False, clamp=structured, engine=engine)
    ds, dn, dwq, dwk, dwv = ops.token_attn_bwd(s, nrm, P["wq"], P["wk"], P["wv"], dopart, into=t("wq", "wk", "wv"),
                                               **({} if drop is None else dict(drop=drop[0])))
    g = dict(wq=dwq, wk=dwk, wv=dwv, wo=dwo, bo=dbo)
    if planes:
        dxf, g["bx"], g["bf"], dws, dbs, dtemp = ops.slice_bwd_points_planes(
            xf, dy, P["ws"], P["bs"], temp, o, ds, dn, nrm, B, N, heads, D, M, engine, clamp=True,
            into=t("bx", "bf", "ws", "bs", "temperature"))
    else:
        dxf, dws, dbs, dtemp = ops.slice_bwd_points(xf, dy, P["ws"], P["bs"], temp, o, ds, dn, B, N, heads, D, M,
                                                    clamp=structured, into=t("ws", "bs", "temperature"), engine=engine)
    dxn, gproj = project_bwd(dxf, kept, P, (H, W), engine, need_dx, t("wx", "bx", "wf", "bf"), planes)
    g.update(gproj, temperature=dtemp.view(1, heads, 1, 1), ws=dws, bs=dbs)
    return dxn, None if T is not None else g


def _attn_targets(params, structured):
    if not structured:
        return None
    tg = grad_targets(params)
    return None if tg is None else dict(zip(ATTN_KEYS, tg))


def _attn_grads(g):
    return tuple(None for _ in ATTN_KEYS) if g is None else tuple(g[k] for k in ATTN_KEYS)


ATTN_KEYS = ("temperature", "wx", "bx", "wf", "bf", "ws", "bs", "wq", "wk", "wv", "wo", "bo")


class PhysicsAttentionFn(Function):
    """out = to_out(deslice(attn(slice(conv(xn))))) (+ res).  H / W: mesh geometry as for attn_forward."""

    @staticmethod
    def forward(ctx, xn, res, H, W, heads, engine, *params):
        P = dict(zip(ATTN_KEYS, (p.detach().contiguous() for p in params)))
        out, saved = attn_forward(xn.detach().contiguous(), P, None if res is None else res.detach().contiguous(),
                                  H, W, heads, engine)
        ctx.P, ctx.saved, ctx.geom, ctx.params = P, saved, (H, W, heads, engine), params
        ctx.has_res = res is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        H, W, heads, engine = ctx.geom
        dout = dout.contiguous()
        dxn, g = attn_backward(ctx.saved, ctx.P, dout, H, W, heads, need_dx=ctx.needs_input_grad[0], engine=engine,
                               targets=_attn_targets(ctx.params, H is not None))
        return (dxn, dout if ctx.has_res else None, None, None, None, None) + _attn_grads(g)


# ------------------------------------------------------------------------------ MLP (Linear-act-Linear)
def mlp_forward(x2d, w1, b1, w2, b2, act, res2d, need_bwd=True, engine=None):
    """need_bwd=False (inference): the pre-activation is not written (one [rows, r*C] store less)."""
    # what is saved is act'(pre-activation): the only use of the pre-activation in the backward (for GELU every term of
    # the derivative is already computed with the activation; the data-gradient epilogue becomes one multiplication)
    hact, hpre = ops.linear_fwd(x2d, w1, b1, act=act, want_pre=need_bwd, engine=engine, save_derivative=True)
    out, _ = ops.linear_fwd(hact, w2, b2, res=res2d, engine=engine)
    return out, (x2d, hpre, hact)


def mlp_backward(saved, w1, w2, act, dout2d, need_dx=True, engine=None, targets=None):
    """`targets` = (dw1, db1, dw2, db2) buffers to add into, or None."""
    x2d, hpre, hact = saved
    t1, t2 = (None, None) if targets is None else (targets[0:2], targets[2:4])
    dhpre = ops.linear_bwd_data(dout2d, w2, pre=hpre, act=act, engine=engine, pre_is_derivative=True)
    dw2, db2 = ops.linear_bwd_weight(dout2d, hact, engine=engine, into=t2)
    dw1, db1 = ops.linear_bwd_weight(dhpre, x2d, engine=engine, into=t1)
    dx = ops.linear_bwd_data(dhpre, w1, engine=engine) if need_dx else None
    return dx, dw1, db1, dw2, db2


class MLPFn(Function):
    """linear_post(act(linear_pre(x))) (+ res) for the n_layers=0 MLP of the reference."""

    @staticmethod
    def forward(ctx, x, res, act, engine, w1, b1, w2, b2):
        shp = x.shape
        ctx.params = (w1, b1, w2, b2)
        x2d = x.detach().reshape(-1, shp[-1]).contiguous()
        w1, b1, w2, b2 = (t.detach().contiguous() for t in (w1, b1, w2, b2))
        res2d = None if res is None else res.detach().reshape(-1, w2.shape[0]).contiguous()
        out, saved = mlp_forward(x2d, w1, b1, w2, b2, act, res2d, need_bwd=any(ctx.needs_input_grad), engine=engine)
        ctx.saved, ctx.w, ctx.act, ctx.shp, ctx.has_res, ctx.engine = saved, (w1, w2), act, shp, res is not None, engine
        return out.view(*shp[:-1], w2.shape[0])

    @staticmethod
    def backward(ctx, dout):
        w1, w2 = ctx.w
        d2 = dout.reshape(-1, w2.shape[0]).contiguous()
        tg = grad_targets(ctx.params)     # None when w1 is the zero-padded copy of a parameter: autograd handles it
        dx, *gw = mlp_backward(ctx.saved, w1, w2, ctx.act, d2, need_dx=ctx.needs_input_grad[0], engine=ctx.engine,
                               targets=tg)
        return (None if dx is None else dx.view(ctx.shp), dout if ctx.has_res else None, None, None) + _ret(tg, gw)


# ------------------------------------------------------------------------------ LayerNorm / head
class LayerNormFn(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta):
        shp = x.shape
        ctx.params = (gamma, beta)
        x2d = x.detach().reshape(-1, shp[-1]).contiguous()
        gamma, beta = gamma.detach().contiguous(), beta.detach().contiguous()
        y, mean, rstd = ops.layernorm_fwd(x2d, gamma, beta)
        ctx.saved, ctx.shp = (x2d, mean, rstd, gamma), shp
        return y.view(shp)

    @staticmethod
    def backward(ctx, dy):
        x2d, mean, rstd, gamma = ctx.saved
        tg = grad_targets(ctx.params)
        dx, dg, db = ops.layernorm_bwd(dy.reshape(x2d.shape).contiguous(), x2d, mean, rstd, gamma, into=tg)
        return (dx.view(ctx.shp),) + _ret(tg, (dg, db))


class HeadFn(Function):
    """mlp2: Linear(C, out_dim <= 8)."""

    @staticmethod
    def forward(ctx, xn, w, b):
        shp = xn.shape
        ctx.params = (w, b)
        x2d = xn.detach().reshape(-1, shp[-1]).contiguous()
        w, b = w.detach().contiguous(), b.detach().contiguous()
        ctx.saved, ctx.shp = (x2d, w), shp
        return ops.head_fwd(x2d, w, b).view(*shp[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2d, w = ctx.saved
        tg = grad_targets(ctx.params)
        dxn, dw, db = ops.head_bwd(dy.reshape(-1, w.shape[0]).contiguous(), x2d, w, into=tg)
        return (dxn.view(ctx.shp),) + _ret(tg, (dw, db))


class AttnBranchFn(Function):
    """fx + Attn(LayerNorm(fx)) as ONE autograd node (Transolver_block.forward, …_2D.py:70): the residual
    gradient is folded into the LayerNorm backward kernel (`dres`), so no separate elementwise add runs.
    H / W: mesh geometry as for attn_forward (W = (width, depth) on the 3-D structured mesh)."""

    @staticmethod
    def forward(ctx, fx, ln_w, ln_b, H, W, heads, engine, dropout, *params):
        shp = fx.shape
        ctx.params, ctx.ln_params = params, (ln_w, ln_b)
        fx2d = fx.detach().reshape(-1, shp[-1]).contiguous()
        ln_w, ln_b = ln_w.detach().contiguous(), ln_b.detach().contiguous()
        P = dict(zip(ATTN_KEYS, (p.detach().contiguous() for p in params)))
        # bf16 engines on fp32 storage: LayerNorm writes the conv's operand planes directly (no fp32 xn, no pre-pass)
        ctx.planes = (H is not None and mesh_extent(W)[1] is None and fx2d.dtype == torch.float32 and len(shp) == 3
                      and ops.conv_planes_mask(shp[0], H, W, shp[2], engine) == 7)
        # training-mode dropout p > 0: the layer's two draws, reserved here (attention, then output) and kept for the backward
        ctx.drop = drop = dropout_draws(dropout, shp[0], shp[1], shp[2], heads, P["ws"].shape[0]) if dropout else None
        if ctx.planes:
            xnp, mean, rstd = ops.layernorm_fwd_planes(fx2d, ln_w, ln_b, engine)
            out, saved = attn_forward(None, P, fx2d.view(shp), H, W, heads, engine, xn_planes=xnp, shape=tuple(shp), drop=drop)
        else:
            xn, mean, rstd = ops.layernorm_fwd(fx2d, ln_w, ln_b)
            out, saved = attn_forward(xn.view(shp), P, fx2d.view(shp), H, W, heads, engine, drop=drop)
        ctx.P, ctx.saved, ctx.geom, ctx.ln = P, saved, (H, W, heads, engine), (fx2d, mean, rstd, ln_w)
        return out

    @staticmethod
    def backward(ctx, dout):
        H, W, heads, engine = ctx.geom
        fx2d, mean, rstd, ln_w = ctx.ln
        dout = dout.contiguous()
        dxn, g = attn_backward(ctx.saved, ctx.P, dout, H, W, heads, need_dx=True, engine=engine,
                               targets=_attn_targets(ctx.params, H is not None), planes=ctx.planes, drop=ctx.drop)
        tl = grad_targets(ctx.ln_params)
        dfx, dg, db = ops.layernorm_bwd(dxn.reshape(fx2d.shape), fx2d, mean, rstd, ln_w, dres=dout.reshape(fx2d.shape),
                                        into=tl)
        return (dfx.view(dout.shape),) + _ret(tl, (dg, db)) + (None, None, None, None, None) + _attn_grads(g)


class MLPBranchFn(Function):
    """fx + MLP(LayerNorm(fx)) as one autograd node (…_2D.py:71), residual gradient folded into LN backward."""

    @staticmethod
    def forward(ctx, fx, ln_w, ln_b, act, engine, w1, b1, w2, b2):
        shp = fx.shape
        ctx.params, ctx.ln_params = (w1, b1, w2, b2), (ln_w, ln_b)
        fx2d = fx.detach().reshape(-1, shp[-1]).contiguous()
        ln_w, ln_b, w1, b1, w2, b2 = (t.detach().contiguous() for t in (ln_w, ln_b, w1, b1, w2, b2))
        xn, mean, rstd = ops.layernorm_fwd(fx2d, ln_w, ln_b)
        out, saved = mlp_forward(xn, w1, b1, w2, b2, act, fx2d, need_bwd=any(ctx.needs_input_grad), engine=engine)
        ctx.saved, ctx.w, ctx.act, ctx.ln, ctx.engine = saved, (w1, w2), act, (fx2d, mean, rstd, ln_w), engine
        return out.view(shp)

    @staticmethod
    def backward(ctx, dout):
        w1, w2 = ctx.w
        fx2d, mean, rstd, ln_w = ctx.ln
        d2 = dout.reshape(fx2d.shape).contiguous()
        tg, tl = grad_targets(ctx.params), grad_targets(ctx.ln_params)
        dxn, *gw = mlp_backward(ctx.saved, w1, w2, ctx.act, d2, need_dx=True, engine=ctx.engine, targets=tg)
        dfx, dg, db = ops.layernorm_bwd(dxn, fx2d, mean, rstd, ln_w, dres=d2, into=tl)
        return (dfx.view(dout.shape),) + _ret(tl, (dg, db)) + (None, None) + _ret(tg, gw)


def block_tail(fx, xn, P, H, W, heads, ln2_w, ln2_b, act, w1, b1, w2, b2, next_w=None, next_b=None, engine=None):
    """One block of a no-grad forward on the fused tail: conv (or the stacked Linear of the irregular mesh), slice
    scatter, token attention, then ops.block_tail_fwd — four library calls.  fx [B,N,C]: the residual stream; xn = ln_1(fx),
    made by the previous block's tail (or by the caller for the first block); P: dict ATTN_KEYS -> tensors; next_w / next_b:
    the LayerNorm that follows (the next block's ln_1, or ln_3).  Returns (fx', LN_next(fx') or None).  No autograd node:
    raises if grad mode is on and an input requires a gradient."""
    tensors = (fx, xn, ln2_w, ln2_b, w1, b1, w2, b2, next_w, next_b) + tuple(P.values())
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise RuntimeError("functional.block_tail has no backward: call it under torch.no_grad()")
    B, N, C = fx.shape
    D, M = C // heads, P["ws"].shape[0]
    c = lambda t: None if t is None else t.detach().contiguous()
    P = {k: c(v) for k, v in P.items()}
    xf, _, _, _, o, temp = _front(c(xn), P, (H, W), heads, engine)
    out, xnext, _ = ops.block_tail_fwd(xf, 2 * C, 0, o, P["ws"], P["bs"], temp, c(fx).view(B * N, C), P["wo"], P["bo"],
                                       c(ln2_w), c(ln2_b), c(w1), c(b1), c(w2), c(b2), c(next_w), c(next_b), B, N, heads,
                                       D, M, act, clamp=H is not None, engine=engine)
    return out.view(B, N, C), None if xnext is None else xnext.view(B, N, C)


def attn_branch(fx, ln_w, ln_b, H, W, heads, params, engine=None, dropout=None):
    """dropout: probability p in (0, 1) of training-mode dropout at the layer's two sites (None or 0: none, and the launches
    of a model without dropout); fp32 storage only."""
    if dropout and fx.dtype != torch.float32:
        raise NotImplementedError("dropout > 0 is served for fp32 storage only")
    return AttnBranchFn.apply(fx, ln_w, ln_b, H, W, heads, engine, dropout or None, *params)


def mlp_branch(fx, ln_w, ln_b, act, w1, b1, w2, b2, engine=None):
    return MLPBranchFn.apply(fx, ln_w, ln_b, act, engine, w1, b1, w2, b2)


class LinearFn(Function):
    """y = act(x . w^T + b): generic dense layer (MLP hidden layers when n_layers > 0, wide heads)."""

    @staticmethod
    def forward(ctx, x, act, engine, w, b):
        shp = x.shape
        x2d = x.detach().reshape(-1, shp[-1]).contiguous()
        w = w.detach().contiguous()
        b = None if b is None else b.detach().contiguous()
        y, pre = ops.linear_fwd(x2d, w, b, act=act, want_pre=act is not None, engine=engine)
        ctx.saved, ctx.act, ctx.shp, ctx.has_b, ctx.engine = (x2d, w, pre), act, shp, b is not None, engine
        return y.view(*shp[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2d, w, pre = ctx.saved
        d2 = dy.reshape(-1, w.shape[0]).contiguous()
        if ctx.act is not None:
            d2 = ops.act_bwd(d2, pre, ctx.act)
        dw, db = ops.linear_bwd_weight(d2, x2d, want_bias=ctx.has_b, engine=ctx.engine)
        dx = ops.linear_bwd_data(d2, w, engine=ctx.engine).view(ctx.shp) if ctx.needs_input_grad[0] else None
        return dx, None, None, dw, db


def linear(x, w, b, act, engine=None):
    return LinearFn.apply(x, act, engine, w, b)


class ActivationFn(Function):
    """act(x) element-wise with the function of the GEMM epilogues (ops.act_fwd / ops.act_bwd)."""

    @staticmethod
    def forward(ctx, x, act):
        pre = x.detach().contiguous()
        ctx.saved, ctx.act = pre, act
        return ops.act_fwd(pre, act)

    @staticmethod
    def backward(ctx, dy):
        return ops.act_bwd(dy.contiguous(), ctx.saved, ctx.act), None


def activation(x, act):
    return x if act is None else ActivationFn.apply(x, act)


def layer_norm(x, gamma, beta):
    return LayerNormFn.apply(x, gamma, beta)


def physics_attention(xn, res, H, W, heads, params, engine=None):
    return PhysicsAttentionFn.apply(xn, res, H, W, heads, engine, *params)


def mlp(x, res, act, w1, b1, w2, b2, engine=None):
    return MLPFn.apply(x, res, act, engine, w1, b1, w2, b2)


def head(xn, w, b):
    return HeadFn.apply(xn, w, b)


class RelL2Fn(Function):
    """Per-sample ||pred-y||_2 / ||y||_2 (utils/testloss.py:31-42) in one kernel; gradient w.r.t. pred."""

    @staticmethod
    def forward(ctx, pred, y):
        B = pred.shape[0]
        p2, y2 = pred.detach().reshape(B, -1).contiguous(), y.detach().reshape(B, -1).contiguous()
        dn, yn, ratio = ops.rel_l2_fwd(p2, y2)
        ctx.saved, ctx.shp = (p2, y2, dn, yn), pred.shape
        return ratio

    @staticmethod
    def backward(ctx, gratio):
        p2, y2, dn, yn = ctx.saved
        # d ratio_b / d pred = (pred - y) / (dn_b * yn_b), times the per-sample upstream gradient (may be 0)
        dpred = ops.rel_l2_bwd(p2, y2, dn, yn, gratio.contiguous())
        return dpred.view(ctx.shp), None


def rel_l2(pred, y):
    return RelL2Fn.apply(pred, y)


class RelL2AffineFn(Function):
    """Per-sample ||o - y|| / ||y|| of the DECODED prediction and target (o = pred std + mean, y = y_n std + mean; mean /
    std the normaliser's one-element device tensors, None = identity) with the target read through its strides
    (ops.rel_l2_affine_fwd / _bwd): the loss of the airfoil, pipe, elasticity and plasticity drivers.  Gradient w.r.t.
    pred only."""

    @staticmethod
    def forward(ctx, pred, y, mean, std):
        B = pred.shape[0]
        L = pred.numel() // max(B, 1)                    # B = 0: an empty [0, 0] problem, the kernels touch nothing
        p2, y = pred.detach().reshape(B, L).contiguous(), y.detach()
        if ops.uniform_strides(y) is None:
            y = y.reshape(B, L).contiguous()
        if mean is not None:
            mean, std = mean.detach().contiguous(), std.detach().contiguous()
        dn, yn, ratio = ops.rel_l2_affine_fwd(p2, y, mean, std)
        ctx.saved, ctx.shp = (p2, y, mean, std, dn, yn), pred.shape
        return ratio

    @staticmethod
    def backward(ctx, gratio):
        p2, y, mean, std, dn, yn = ctx.saved
        dpred = ops.rel_l2_affine_bwd(p2, y, mean, std, dn, yn, gratio.contiguous())
        return dpred.view(ctx.shp), None, None, None


def rel_l2_affine(pred, y, mean=None, std=None):
    return RelL2AffineFn.apply(pred, y, mean, std)


class EmbedBiasFn(Function):
    """z = (h + placeholder[None, None, :]) + tvec[:, None, :] in one launch (ops.embed_bias_fwd); the backward hands dz on
    as dh and makes dplaceholder / dtvec by one fixed-order column reduction (ops.embed_bias_bwd)."""

    @staticmethod
    def forward(ctx, h, placeholder, tvec):
        det = lambda t: None if t is None else t.detach().contiguous()
        ctx.has = (placeholder is not None, tvec is not None)
        return ops.embed_bias_fwd(det(h), det(placeholder), det(tvec))

    @staticmethod
    def backward(ctx, dz):
        want_p = ctx.has[0] and ctx.needs_input_grad[1]
        want_t = ctx.has[1] and ctx.needs_input_grad[2]
        if not (want_p or want_t):
            return dz, None, None
        src = dz.contiguous()
        if src.data_ptr() % 16:          # a view at an odd offset: the reduction reads 16 bytes at a time
            src = src.clone()
        dp, dt = ops.embed_bias_bwd(src, want_p, want_t)
        return dz, dp, dt


def embed_bias(h, placeholder=None, tvec=None):
    """The input embedding's broadcast adds.  Where the kernels do not apply (C % 4 != 0, not fp32 on the GPU) the torch
    expression stays: the same sums in the same order."""
    if (placeholder is None and tvec is None):
        return h
    if not ops.embed_bias_supported(h, placeholder, tvec):
        z = h if placeholder is None else h + placeholder[None, None, :]
        return z if tvec is None else z + tvec[:, None, :]
    return EmbedBiasFn.apply(h, placeholder, tvec)


class DarcyLossFn(Function):
    """The exp_darcy.py:213-226 loss of the normalised prediction `out_n` [B, s*s] against the normalised target `y_n`:
    decode with the y-normaliser's (mean, std) device scalars, rel-L2 plus 0.1 x the rel-L2 of the zero-padded central
    differences of the border-zeroed prediction, in one stencil kernel each way (ops.darcy_loss_fwd / _bwd).
    Returns (loss, sum l2, sum (dxr + dyr)); gradient w.r.t. out_n only."""

    @staticmethod
    def forward(ctx, out_n, y_n, mean, std, dx, s):
        o2, y2 = out_n.detach().contiguous(), y_n.detach().contiguous()
        mean, std = mean.detach().contiguous(), std.detach().contiguous()
        sums, norms = ops.darcy_loss_fwd(o2, y2, mean, std, dx, s)
        ctx.saved, ctx.geom = (o2, y2, mean, std, norms), (dx, s)
        return sums[0], sums[1], sums[2]

    @staticmethod
    def backward(ctx, gloss, gl2, gderiv):
        o2, y2, mean, std, norms = ctx.saved
        coef = torch.stack((gloss + gl2, 0.1 * gloss + gderiv)).to(torch.float32).contiguous()
        dout = ops.darcy_loss_bwd(o2, y2, mean, std, norms, coef, *ctx.geom)
        return dout, None, None, None, None, None


def darcy_loss(out_n, y_n, mean, std, dx, s):
    return DarcyLossFn.apply(out_n, y_n, mean, std, dx, s)


# ------------------------------------------------------------------------------ auto-encoder attention
# Physics_Attention_Structured_Mesh_2D_Auto_Encoder (reference model/Physics_Attention.py): `encode` returns the slice
# tokens after token attention (the code) and caches the softmax slice weights; `reconstruct_fx` / `decode` project the
# cached weights with Linear(M, M) and de-slice the code with them.  The pieces are separate autograd nodes because the
# cached weights are module state that the caller may read, replace or project again between the calls.
ENC_KEYS = ("temperature", "wx", "bx", "wf", "bf", "ws", "bs", "wq", "wk", "wv")


class EncodeFn(Function):
    """xn [B,N,C] (already layer-normed) -> (code [B,heads,M,D], x_mid [B,N,C]): the 3x3 conv pair, slice scatter and
    token attention of the 2-D structured attention.  x_mid is the column view of the conv output (row pitch 2C) that the
    slice-weight node reads.  Backward: token attention backward from dcode, the slice backward with a zero de-slice
    gradient, the x_mid gradient of the slice-weight node added to its x_mid half, then the conv backward."""

    @staticmethod
    def forward(ctx, xn, H, W, heads, engine, *params):
        P = dict(zip(ENC_KEYS, (p.detach().contiguous() for p in params)))
        xn = xn.detach().contiguous()
        B, N, C = xn.shape
        xf, kept, s, nrm, o, temp = _front(xn, P, (H, W), heads, engine)                          # xf [B,N,2C]
        ctx.P, ctx.saved, ctx.geom, ctx.params = P, (kept, xf, s, nrm, o, temp), (H, W, heads, engine), params
        return o.view(B, heads, P["ws"].shape[0], C // heads), xf[:, :, :C]

    @staticmethod
    def backward(ctx, dcode, dxm):
        H, W, heads, engine = ctx.geom
        P = ctx.P
        kept, xf, s, nrm, o, temp = ctx.saved
        B, N, C = kept[2]
        D = C // heads
        M = P["ws"].shape[0]
        tg = grad_targets(ctx.params)
        t = _target_lookup(None if tg is None else dict(zip(ENC_KEYS, tg)))
        dop = (dcode.contiguous() if dcode is not None else torch.zeros_like(o)).view(B * heads, 1, M, D)
        ds, dn, dwq, dwk, dwv = ops.token_attn_bwd(s, nrm, P["wq"], P["wk"], P["wv"], dop, into=t("wq", "wk", "wv"))
        dy0 = torch.zeros(B, N, C, dtype=torch.float32, device=xf.device)
        dxf, dws, dbs, dtemp = ops.slice_bwd_points(xf, dy0, P["ws"], P["bs"], temp, o, ds, dn, B, N, heads, D, M,
                                                    clamp=True, into=t("ws", "bs", "temperature"), engine=engine)
        if dxm is not None:
            dxf[:, :, :C] += dxm
        dxn, g = project_bwd(dxf, kept, P, (H, W), engine, ctx.needs_input_grad[0], t("wx", "bx", "wf", "bf"), False)
        g.update(temperature=dtemp.view(1, heads, 1, 1), ws=dws, bs=dbs, wq=dwq, wk=dwk, wv=dwv)
        return (dxn, None, None, None, None) + tuple(None if tg is not None else g[k] for k in ENC_KEYS)


class SliceWeightsFn(Function):
    """sw [B,heads,N,M] = softmax((x_mid . Ws^T + bs) / clamp(temperature, 0.1, 5)) per head (pa2d_slice_weights_*)."""

    @staticmethod
    def forward(ctx, xm, temperature, ws, bs):
        heads = temperature.numel()
        ctx.params = (temperature, ws, bs)
        temp = temperature.detach().reshape(heads).contiguous()
        ws, bs = ws.detach().contiguous(), bs.detach().contiguous()
        xm = xm.detach()
        ctx.saved = (xm, temp, ws, bs)
        return ops.slice_weights_fwd(xm, ws, bs, temp, heads)

    @staticmethod
    def backward(ctx, dsw):
        xm, temp, ws, bs = ctx.saved
        heads = temp.numel()
        tg = grad_targets(ctx.params)
        into = None if tg is None else (tg[1], tg[2], tg[0])
        dxm, dws, dbs, dtemp = ops.slice_weights_bwd(xm, ws, bs, temp, dsw.contiguous(), need_dx=ctx.needs_input_grad[0],
                                                     into=into)
        return (dxm,) + _ret(tg, (dtemp.view(1, heads, 1, 1), dws, dbs))


class DesliceWeightsFn(Function):
    """y [B,N,heads*D] = einsum("bhgc,bhng->bhnc", code, w) rearranged to [B,N,(h d)] (pa2d_deslice_weights_*)."""

    @staticmethod
    def forward(ctx, code, w):
        code, w = code.detach().contiguous(), w.detach().contiguous()
        ctx.saved = (code, w)
        return ops.deslice_weights_fwd(code, w)

    @staticmethod
    def backward(ctx, dy):
        code, w = ctx.saved
        return ops.deslice_weights_bwd(code, w, dy.contiguous(), need_dcode=ctx.needs_input_grad[0],
                                       need_dw=ctx.needs_input_grad[1])


class ToOutTwiceFn(Function):
    """2 * to_out(y): the auto-encoder's last block adds reconstruct_fx(code) and decode(code), which are the same
    to_out(deslice(code, P(sw))).  One GEMM with the weight and bias doubled (exact: every product and partial sum
    scales by 2), so the result is bit for bit what the reference's sum is."""

    @staticmethod
    def forward(ctx, y, engine, w, b):
        shp = y.shape
        y2d = y.detach().reshape(-1, shp[-1]).contiguous()
        w2, b2 = 2.0 * w.detach(), 2.0 * b.detach()
        with ops.unscoped():      # the doubled weight is a temporary: a weights_frozen() scope gets no entry for it
            out, _ = ops.linear_fwd(y2d, w2, b2, engine=engine)
        ctx.saved, ctx.shp, ctx.engine = (y2d, w2), shp, engine
        return out.view(*shp[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dout):
        y2d, w2 = ctx.saved
        d2 = dout.reshape(-1, w2.shape[0]).contiguous()
        dy = dw = db = None
        if ctx.needs_input_grad[0]:
            with ops.unscoped():
                dy = ops.linear_bwd_data(d2, w2, engine=ctx.engine).view(ctx.shp)
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            dw, db = ops.linear_bwd_weight(d2, y2d, engine=ctx.engine)
            dw.mul_(2.0)
            db.mul_(2.0)
        return dy, None, dw, db


def attention_encode(xn, H, W, heads, params, engine=None):
    """(code, x_mid) of the auto-encoder attention; `params` in ENC_KEYS order."""
    return EncodeFn.apply(xn, H, W, heads, engine, *params)


def slice_weights(xm, temperature, ws, bs):
    return SliceWeightsFn.apply(xm, temperature, ws, bs)


def deslice_weights(code, w):
    """Public de-slice with an explicit weight tensor: code [B,heads,M,D], w [B,heads,N,M] -> [B,N,heads*D]
    (the reference's einsum("bhgc,bhng->bhnc") + rearrange; for callers such as the SequenSolver drivers)."""
    return DesliceWeightsFn.apply(code, w)


def to_out_twice(y, w, b, engine=None):
    return ToOutTwiceFn.apply(y, engine, w, b)


# ------------------------------------------------------------------------------ SequenSolver stages
class SeqAttnFn(Function):
    """out [B,T,dim] = softmax(q k^T * scale) v (+ res) among the T frame tokens of a sample (SequenSolver.attention,
    SequenSolver.py:325-328, and the `+ tokens` of :150; pa2d_seq_attn_*).  The [B,T,T] attention matrix is saved for
    the backward."""

    @staticmethod
    def forward(ctx, q, k, v, res, scale, causal=False):
        q, k, v = (t.detach().contiguous() for t in (q, k, v))
        out, attn = ops.seq_attn_fwd(q, k, v, scale, res=None if res is None else res.detach().contiguous(), causal=causal)
        ctx.saved, ctx.scale, ctx.has_res, ctx.causal = (q, k, v, attn), scale, res is not None, causal
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, attn = ctx.saved
        dout = dout.contiguous()
        return ops.seq_attn_bwd(q, k, v, attn, dout, ctx.scale, causal=ctx.causal) + (dout if ctx.has_res else None, None,
                                                                                     None)


def seq_attention(q, k, v, scale, res=None, causal=False):
    """Single-head attention among T <= 32 tokens of width dim <= 1024 (dim % 4 == 0): q, k, v [B, T, dim]; `res`
    [B, T, dim] is added to the result in the kernel's epilogue.  `causal`: token i attends to the tokens j <= i."""
    return SeqAttnFn.apply(q, k, v, res, scale, bool(causal))


class HeadSeqAttnFn(Function):
    """The merged SequenSolver's attention on x [G, T, sd] (G = B*heads groups of the LayerNorm output) as ONE node and one
    forward launch: the three shared Linear(sd, sd), the (causal) softmax attention and the residual
    (pa2d_head_seq_attn_*).  Only x and the [G, T, T] attention matrix are kept; the backward recomputes q, k, v."""

    @staticmethod
    def forward(ctx, x, res, scale, causal, wq, wk, wv):
        ctx.params = (wq, wk, wv)
        x = x.detach().contiguous()
        W = tuple(w.detach().contiguous() for w in (wq, wk, wv))
        out, attn = ops.head_seq_attn_fwd(x, *W, scale, res=None if res is None else res.detach().contiguous(),
                                          causal=causal)
        ctx.saved, ctx.scale, ctx.causal, ctx.has_res = (x, W, attn), scale, causal, res is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        x, W, attn = ctx.saved
        dout = dout.contiguous()
        tg = grad_targets(ctx.params)
        dx, *g = ops.head_seq_attn_bwd(x, *W, attn, dout, ctx.scale, causal=ctx.causal, into=tg)
        return (dx, dout if ctx.has_res else None, None, None) + _ret(tg, g)


def head_seq_attention(xn, wq, wk, wv, heads, scale, res=None, causal=True, engine=None, fused=None):
    """Attention of the merged SequenSolver: xn [B, T, dim] (already layer-normed) is read, as contiguous memory, as
    [B*heads, T, sd] with sd = dim // heads; wq, wk, wv [sd, sd] are shared by all groups; `res` [B, T, dim] is added in
    the kernel's epilogue.  Returns [B, T, dim].  fused=None: the fused kernel where sd <= ops.HEAD_SEQ_ATTN_MAX_SD, else
    three `linear` and a causal `seq_attention` on the [B*heads, T, sd] view (fused=False forces that route; fused=True
    raises where the fused kernel does not serve the shape).  `engine` is the GEMM engine of the unfused route's linears;
    the fused kernel is exact fp32 on every engine."""
    B, T, dim = xn.shape
    if heads < 1 or dim % heads:
        raise ValueError(f"heads = {heads} must divide dim = {dim}")
    sd = dim // heads
    x = xn.reshape(B * heads, T, sd)
    r = None if res is None else res.reshape(B * heads, T, sd)
    if fused is None:
        fused = sd <= ops.HEAD_SEQ_ATTN_MAX_SD
    if fused:
        out = HeadSeqAttnFn.apply(x, r, scale, bool(causal), wq, wk, wv)
    else:
        q, k, v = (linear(x, w, None, None, engine=engine) for w in (wq, wk, wv))
        out = seq_attention(q, k, v, scale, res=r, causal=causal)
    return out.reshape(B, T, dim)


def code_slice_weights(code, pos, w1, b1, w2, b2, w3, b3):
    """code [B, M, C], pos [B, N, 2] and the six tensors of weight_projection = MLP(C+2, 64, 1) -> sw [B, 1, N, M]."""
    ops._two_coordinates(code, pos)
    return PointSliceWeightsFn.apply(code, pos, w1, b1, w2, b2, w3, b3)


# ------------------------------------------------------------------------------ LearnSlice stages
class PointSliceWeightsFn(Function):
    """sw [B,1,N,M] = softmax_M(weight_projection(cat(code_m, feat_n))) with P features per point (LearnSlice.py:100-153;
    pa2d_point_slice_weights_*).  The features get no gradient."""

    @staticmethod
    def forward(ctx, code, feat, *params):
        ctx.params = params
        code, feat = code.detach().contiguous(), feat.detach().contiguous()
        P = tuple(p.detach().contiguous() for p in params)
        ctx.saved = (code, feat, P)
        return ops.point_slice_weights_fwd(code, feat, P)

    @staticmethod
    def backward(ctx, dsw):
        code, feat, P = ctx.saved
        tg = grad_targets(ctx.params)
        dcode, *g = ops.point_slice_weights_bwd(code, feat, P, dsw.contiguous(), need_dcode=ctx.needs_input_grad[0], into=tg)
        return (dcode, None) + _ret(tg, g)


class SliceMSEFn(Function):
    """loss (0-dim) = sum over the rows of mean_m (sw - target)^2: the reference trainer's sum over the points of
    F.mse_loss(w_n, target_n) (LearnSlice.py:499-510; pa2d_slice_mse_*).  Gradient w.r.t. sw only."""

    @staticmethod
    def forward(ctx, sw, target):
        sw, target = sw.detach().contiguous(), target.detach().contiguous()
        ctx.saved = (sw, target)
        return ops.slice_mse_fwd(sw, target).reshape(())

    @staticmethod
    def backward(ctx, gout):
        sw, target = ctx.saved
        return ops.slice_mse_bwd(sw, target, gout.reshape(1).contiguous()), None


def point_slice_weights(code, feat, w1, b1, w2, b2, w3, b3):
    """code [B, M, C], feat [B, N, P] (1 <= P <= 128) and the six tensors of weight_projection = MLP(C+P, 64, 1)
    -> sw [B, 1, N, M]."""
    return PointSliceWeightsFn.apply(code, feat, w1, b1, w2, b2, w3, b3)


def slice_mse(sw, target):
    """sw, target [..., M] -> the 0-dim loss sum_rows mean_m (sw - target)^2."""
    return SliceMSEFn.apply(sw, target)


# ------------------------------------------------------------------------------ conv slice predictors
class Conv3x3Fn(Function):
    """One Conv2d(C, C, 3, 1, 1) on the [B, N, C] tensor (pa2d_conv3x3_*): in_project_x of the conv slice predictors."""

    @staticmethod
    def forward(ctx, xn, H, W, engine, w, b):
        ctx.params = (w, b)
        xn = xn.detach().contiguous()
        w, b = w.detach().contiguous(), b.detach().contiguous()
        ctx.saved, ctx.geom = (xn, w), (H, W, engine)
        return ops.conv3x3_fwd(xn, w, b, H, W, engine=engine)

    @staticmethod
    def backward(ctx, dout):
        xn, w = ctx.saved
        H, W, engine = ctx.geom
        tg = grad_targets(ctx.params)
        dxn, dw, db = ops.conv3x3_bwd(dout.contiguous(), xn, w, H, W, need_dx=ctx.needs_input_grad[0], engine=engine,
                                      into=tg)
        return (dxn, None, None, None) + _ret(tg, (dw, db))


def _constant_pitch(x):
    """x as the row-pitch stages take it: itself where its rows sit at one pitch (a column view), else a contiguous copy
    (an expanded gradient, a permuted tensor)."""
    if x.is_contiguous():
        return x
    try:
        ops._rows_view(x)
    except ValueError:
        return x.contiguous()
    return x


class ZScoreFn(Function):
    """(x - x.mean()) / (x.std(unbiased=False) + 1e-8) over the whole tensor, batch included (pa2d_zscore_*)."""

    @staticmethod
    def forward(ctx, x):
        y, stats = ops.zscore_fwd(_constant_pitch(x.detach()))
        ctx.saved = (y, stats)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, stats = ctx.saved
        return ops.zscore_bwd(_constant_pitch(dy), y, stats)


class GroupedZScoreFn(Function):
    """ZScoreFn over `groups` runs of consecutive leading entries, one set of statistics each (pa2d_zscore_grouped_*)."""

    @staticmethod
    def forward(ctx, x, groups):
        y, stats = ops.zscore_grouped_fwd(_constant_pitch(x.detach()), groups)
        ctx.saved = (y, stats)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, stats = ctx.saved
        return ops.zscore_grouped_bwd(_constant_pitch(dy), y, stats), None


class WideSliceWeightsFn(Function):
    """sw [..., M] = softmax((x . Ws^T + bs) / clamp(temperature, 0.1, 5)) for rows of 16..512 features
    (pa2d_wide_slice_weights_*); the weights are recomputed in the backward, never saved."""

    @staticmethod
    def forward(ctx, x, temperature, ws, bs):
        ctx.params = (temperature, ws, bs)
        temp = temperature.detach().reshape(1).contiguous()
        ws, bs = ws.detach().contiguous(), bs.detach().contiguous()
        x = _constant_pitch(x.detach())
        ctx.saved, ctx.tshape = (x, temp, ws, bs), temperature.shape
        return ops.wide_slice_weights_fwd(x, ws, bs, temp)

    @staticmethod
    def backward(ctx, dsw):
        x, temp, ws, bs = ctx.saved
        tg = grad_targets(ctx.params)
        into = None if tg is None else (tg[1], tg[2], tg[0])
        dx, dws, dbs, dtemp = ops.wide_slice_weights_bwd(x, ws, bs, temp, dsw.contiguous(), need_dx=ctx.needs_input_grad[0],
                                                         into=into)
        return (dx,) + _ret(tg, (dtemp.view(ctx.tshape), dws, dbs))


def conv3x3(xn, H, W, w, b, engine=None):
    """[B, N, C] -> Conv2d(C, C, 3, 1, 1) of the [B, H, W, C] image, as [B, N, C]."""
    return Conv3x3Fn.apply(xn, H, W, engine, w, b)


def zscore(x, groups=1):
    """groups > 1: x.shape[0] is cut into `groups` runs of consecutive entries, each z-scored on its own (what `groups`
    separate calls on those runs give, bit for bit, in one pair of launches); groups = 1 is the whole-tensor node."""
    if groups == 1:
        return ZScoreFn.apply(x)
    if groups < 1 or x.dim() < 2 or x.shape[0] % groups:
        raise ValueError(f"groups = {groups} must divide the leading dimension of {tuple(x.shape)}")
    return GroupedZScoreFn.apply(x, groups)


def wide_slice_weights(x, temperature, ws, bs):
    """x [..., D] -> [..., M]; temperature holds one scalar (any shape), clamped to [0.1, 5]."""
    return WideSliceWeightsFn.apply(x, temperature, ws, bs)


class PrevSliceEntryFn(Function):
    """h0 = act(sw . wsw^T + tb[:, None, :]) in one launch (ops.prev_slice_entry_fwd): the first layer of the previous-slice
    predictor.  Backward (ops.prev_slice_entry_bwd): one kernel (M > 16: ceil(M / 16) grid slices of it, each reading dh0) and
    the two fixed-order sums of its partial records.  The backward recomputes the pre-activation; gradients of wsw and tb only (sw is data)."""

    @staticmethod
    def forward(ctx, sw, wsw, tb, act):
        sw, wsw, tb = sw.detach().contiguous(), wsw.detach().contiguous(), tb.detach().contiguous()
        ctx.saved, ctx.act = (sw, wsw, tb), act
        return ops.prev_slice_entry_fwd(sw, wsw, tb, act)

    @staticmethod
    def backward(ctx, dh0):
        sw, wsw, tb = ctx.saved
        src = dh0.contiguous()
        if src.data_ptr() % 16:          # a view at an odd offset: the kernel reads 16 bytes at a time
            src = src.clone()
        dwsw, dtb = ops.prev_slice_entry_bwd(src, sw, wsw, tb, ctx.act)
        return None, dwsw, dtb, None


def prev_slice_entry(sw, wsw, tb, act, fused=True, engine=None):
    """First layer of the previous-slice predictor without the [B, N, M + M C] concatenation: sw [B, N, M] (the points'
    slice weights, data), wsw [H, M] (the weight columns that multiply them), tb [B, H] (the code columns' product plus the
    bias, one row per sample) -> act(sw . wsw^T + tb[b]) [B, N, H].
    fused=True: pa2d_prev_slice_entry_* (one launch forward; one kernel and two record sums backward), exact fp32.  fused=False: the three-op route the other
    predictors take for a per-sample row — the row GEMM on `engine`, the broadcast add, the activation."""
    if sw.requires_grad:
        raise ValueError("prev_slice_entry takes the slice weights as data: no gradient flows to `sw` "
                         "(detach it, as the trainers' frozen encoder does)")
    if fused:
        return PrevSliceEntryFn.apply(sw, wsw, tb, act)
    rem = wsw.shape[1] % 4                      # the GEMMs load 16 bytes at a time along the contraction
    if rem:
        sw, wsw = torch.nn.functional.pad(sw, (0, 4 - rem)), torch.nn.functional.pad(wsw, (0, 4 - rem))
    if tb.shape[-1] % 4:
        raise NotImplementedError(f"prev_slice_entry needs a hidden width that is a multiple of 4; got {tb.shape[-1]}")
    return activation(embed_bias(linear(sw, wsw, None, None, engine=engine), None, tb), act)


class RelL2WindowFn(Function):
    """Per-sample ||pred - yy[..., col0:col0+k]|| / ||yy[..., col0:col0+k]|| of pred [B, N, k] with the column window of
    the wider target read in place (ops.rel_l2_window_fwd / _bwd): the loss of the velocity-field trainers, whose
    prediction is a (vel_x, vel_y) pair.  Gradient w.r.t. pred only."""

    @staticmethod
    def forward(ctx, pred, yy, col0):
        p3, yy = pred.detach().contiguous(), yy.detach()
        dn, yn, ratio = ops.rel_l2_window_fwd(p3, yy, col0)
        ctx.saved, ctx.col0 = (p3, yy, dn, yn), col0
        return ratio

    @staticmethod
    def backward(ctx, gratio):
        p3, yy, dn, yn = ctx.saved
        return ops.rel_l2_window_bwd(p3, yy, ctx.col0, dn, yn, gratio.contiguous()), None, None


def rel_l2_window(pred, yy, col0, k):
    """ratio [B] of pred [B, N, k] against the columns [col0, col0 + k) of yy [B, N, W] (fp32 GPU tensors; yy may be a view
    with unit stride along its last axis).  `k` must be pred's last dimension."""
    if pred.dim() != 3 or pred.shape[-1] != k:
        raise ValueError(f"rel_l2_window needs pred [B, N, {k}]; got {tuple(pred.shape)}")
    return RelL2WindowFn.apply(pred, yy, col0)
