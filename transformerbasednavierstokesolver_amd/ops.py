"""Stage-level wrappers over the libpa2d C ABI.

PyTorch is used here only as plumbing: it owns device memory (outputs and workspaces come from the
caching allocator, so nothing is allocated inside the native calls) and provides the current HIP
stream.  Every function takes contiguous fp32 CUDA(HIP) tensors and raises otherwise — there is no
CPU path (the CPU restatement lives in oracle/ and is test infrastructure only).

Parameter-gradient outputs: every backward op takes `into=` — a tuple of existing gradient buffers (the
views of the flat gradient bucket) that the kernels ADD to (`accumulate = 1` in the C ABI); without it the
op allocates fresh tensors and overwrites them.

Weight packs and images: inside `weights_frozen()` everything derived from a weight (conv packs, GEMM weight images, the
fused tail's images) is made once and kept in the scope's one table (`_scoped`); outside a scope each call derives it in its
own workspace.  `weights_frozen(scope)` enters a kept scope again, with the entries it already holds.  Under `unscoped()` a
call behaves as outside any scope: for calls on a temporary weight, which a scope would keep alive and never hit again.
"""
from __future__ import annotations

from types import MappingProxyType
from typing import NamedTuple

import torch

from . import _lib

ACT_IDS = {None: 0, "none": 0, "gelu": 1, "tanh": 2, "sigmoid": 3, "relu": 4, "softplus": 5, "ELU": 6, "silu": 7}
LN_EPS = 1e-5


# Optional provider of (hipEvent_t start, hipEvent_t stop) handles, called as provider(kind) with kind in
# {"conv", "slice_scatter", "deslice", "slice_bwd"}; libpa2d records them on the launch stream right around that
# kernel (bench.py installs one to time the roofline kernels live); None = off.
event_provider = None


def _events(kind):
    return event_provider(kind) if event_provider is not None else (0, 0)


# GEMM engines (include/pa2d.h: enum pa2d_engine).  The engine is an explicit argument of every dense op; `None`
# means pa2d_default_engine() (env PA2D_GEMM=f32|split|bf16, else the fp32-accurate split engine).
ENGINE_F32, ENGINE_SPLIT, ENGINE_BF16 = 0, 1, 2
# bf16 STORAGE (BASELINE configs[2] / [4] as stated): not an engine id of the C ABI but a host-side mode — the blocks'
# activations, saved tensors and inter-kernel gradients are torch.bfloat16 tensors, and every op below dispatches on the
# activation dtype to the *_bf16 entry points (one-term bf16 MFMA, fp32 accumulate, fp32 parameters / statistics).
# fp32-in/fp32-out calls made by a model in this mode (the input embedding) run on ENGINE_BF16.
ENGINE_BF16S = 3
ENGINE_NAMES = {"f32": ENGINE_F32, "split": ENGINE_SPLIT, "bf16": ENGINE_BF16, "bf16s": ENGINE_BF16S}


def default_engine():
    import os
    if os.environ.get("PA2D_GEMM", "") == "bf16s":      # host-side mode (see ENGINE_BF16S), not an ABI engine
        return ENGINE_BF16S
    return _L().pa2d_default_engine()


def resolve_engine(engine):
    if engine is None:
        return default_engine()
    if isinstance(engine, str):
        return ENGINE_NAMES[engine]
    if engine not in (ENGINE_F32, ENGINE_SPLIT, ENGINE_BF16, ENGINE_BF16S):
        raise ValueError(f"unknown GEMM engine {engine!r}")
    return int(engine)


def _abi_engine(engine):
    """Engine id for an fp32-I/O entry point of the C ABI (bf16-storage models run those on the bf16-compute engine)."""
    eng = resolve_engine(engine)
    return ENGINE_BF16 if eng == ENGINE_BF16S else eng


def _L():
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _chk(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("libpa2d ops need tensors on the GPU (no CPU fallback exists in this package)")
        if t.dtype != torch.float32:
            raise TypeError(f"libpa2d ops are fp32; got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError("libpa2d ops need contiguous tensors")


def _chk_act(*ts):
    """Activation tensors: contiguous GPU fp32 or bf16, all of ONE dtype.  Returns True for bf16 storage."""
    dt = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("libpa2d ops need tensors on the GPU (no CPU fallback exists in this package)")
        if t.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"libpa2d activations are fp32 or bf16; got {t.dtype}")
        if dt is not None and t.dtype != dt:
            raise TypeError(f"activation tensors of one op must share a storage type; got {dt} and {t.dtype}")
        dt = t.dtype
        if not t.is_contiguous():
            raise ValueError("libpa2d ops need contiguous tensors")
    return dt == torch.bfloat16


def _p(t, offset_elems=0):
    return 0 if t is None else t.data_ptr() + t.element_size() * offset_elems


def _fn(name, bf):
    return getattr(_L(), name + "_bf16" if bf else name)


def _ws(nbytes, like):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=like.device)


def _grad_outputs(into, shapes, like):
    """(tensors, accumulate flag): the caller's buffers (added to) or fresh ones (overwritten)."""
    if into is not None:
        if len(into) != len(shapes):
            raise ValueError("`into` must hold one buffer per gradient output")
        for t, shp in zip(into, shapes):
            _chk(t)
            if t.numel() != int(torch.Size(shp).numel()):
                raise ValueError("gradient buffer of the wrong size")
        return tuple(into), 1
    return tuple(torch.empty(shp, dtype=torch.float32, device=like.device) for shp in shapes), 0


# ----------------------------------------------------------------------------------------------
def layernorm_fwd(x2d, gamma, beta, eps=LN_EPS):
    _chk(gamma, beta)
    bf = _chk_act(x2d)
    rows, Cc = x2d.shape
    y = torch.empty_like(x2d)
    mean = torch.empty(rows, dtype=torch.float32, device=x2d.device)
    rstd = torch.empty_like(mean)
    _lib.check(_fn("pa2d_layernorm_fwd", bf)(_p(x2d), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), rows, Cc, eps,
                                       _stream()), "layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(dy, x2d, mean, rstd, gamma, dres=None, into=None):
    _chk(mean, rstd, gamma)
    bf = _chk_act(dy, x2d, dres)
    rows, Cc = x2d.shape
    dx = torch.empty_like(x2d)
    (dg, db), acc = _grad_outputs(into, (gamma.shape, gamma.shape), x2d)
    nb = _L().pa2d_layernorm_bwd_workspace(rows, Cc)
    ws = _ws(nb, x2d)
    _lib.check(_fn("pa2d_layernorm_bwd", bf)(_p(dy), _p(x2d), _p(mean), _p(rstd), _p(gamma), _p(dres), _p(dx), _p(dg),
                                       _p(db), ws.data_ptr(), nb, rows, Cc, acc, _stream()), "layernorm_bwd")
    return dx, dg, db


ACT_SAVE_DERIVATIVE = 0x100      # include/pa2d.h: PA2D_ACT_SAVE_DERIVATIVE


def _make_image(img, w, transposed, N, K, eng):
    """Plane image of w for the row-stationary linear kernel; N, K: the GEMM's output width and contraction length (forward:
    the layer's [N, K]; data gradient: [K, N])."""
    _lib.check(_L().pa2d_gemm_weight_image(_p(w), w.shape[1], transposed, img.data_ptr(), img.numel(), N, K, eng, _stream()),
               "gemm_weight_image")


def linear_fwd(x2d, w, bias=None, res=None, act=None, want_pre=False, engine=None, save_derivative=False):
    """y = act(x . w^T + bias) (+ res); returns (y, pre) with pre = pre-activation if want_pre — or act'(pre-activation)
    with save_derivative (what `linear_bwd_data(..., pre_is_derivative=True)` multiplies by)."""
    _chk(w, bias)
    bf = _chk_act(x2d, res)
    M, K = x2d.shape
    N = w.shape[0]
    y = torch.empty(M, N, dtype=x2d.dtype, device=x2d.device)
    pre = torch.empty_like(y) if want_pre else None
    aflag = ACT_SAVE_DERIVATIVE if (save_derivative and want_pre and act is not None) else 0
    if bf:
        _lib.check(_L().pa2d_gemm_bias_act_fwd_bf16(_p(x2d), K, _p(w), w.shape[1], _p(bias), _p(res), N, _p(y), N,
                                                    _p(pre), N, M, N, K, ACT_IDS[act] | aflag, _stream()), "gemm_bias_act_fwd_bf16")
    else:
        eng = _abi_engine(engine)
        nb = _L().pa2d_gemm_fwd_workspace(N, K, eng)
        # inside weights_frozen(): the weight image is made once per weight (0 = the call makes it in its scratch)
        img = _scoped(("image", w.data_ptr(), 0, N, K, eng), nb, _make_image, (w,), w, 0, N, K, eng)
        ws = _ws(nb, x2d) if (nb and not img) else None
        _lib.check(_L().pa2d_gemm_bias_act_fwd(_p(x2d), K, _p(w), w.shape[1], _p(bias), _p(res), N, _p(y), N, _p(pre), N,
                                               img, _p(ws), nb if ws is not None else 0, M, N, K, ACT_IDS[act] | aflag, eng,
                                               _stream()), "gemm_bias_act_fwd")
    return y, pre


def linear_bwd_data(dy, w, pre=None, act=None, engine=None, pre_is_derivative=False):
    """dx = (dy . w) * act'(pre); pre_is_derivative: `pre` already holds act'(pre-activation) (linear_fwd(save_derivative=True))."""
    _chk(w)
    bf = _chk_act(dy, pre)
    M, N = dy.shape
    K = w.shape[1]
    dx = torch.empty(M, K, dtype=dy.dtype, device=dy.device)
    aflag = ACT_SAVE_DERIVATIVE if (pre_is_derivative and pre is not None and act is not None) else 0
    if bf:
        wt = torch.empty(K * N, dtype=torch.float32, device=dy.device)
        _lib.check(_L().pa2d_gemm_bwd_data_bf16(_p(dy), N, _p(w), K, _p(pre), K, ACT_IDS[act] | aflag, _p(dx), K, _p(wt), M, N, K,
                                                _stream()), "gemm_bwd_data_bf16")
    else:
        eng = _abi_engine(engine)
        nimg = _L().pa2d_gemm_fwd_workspace(K, N, eng)     # the data gradient is a GEMM of output width K, contraction N
        img = _scoped(("image", w.data_ptr(), 1, K, N, eng), nimg, _make_image, (w,), w, 1, K, N, eng)
        nb = _L().pa2d_gemm_bwd_data_workspace(N, K, eng) - (nimg if img else 0)      # [transposed weight | image unless ready-made]
        ws = _ws(nb, dy)
        _lib.check(_L().pa2d_gemm_bwd_data(_p(dy), N, _p(w), K, _p(pre), K, ACT_IDS[act] | aflag, _p(dx), K, img, ws.data_ptr(), nb,
                                           M, N, K, eng, _stream()), "gemm_bwd_data")
    return dx


def linear_bwd_weight(dy, x2d, want_bias=True, engine=None, into=None):
    """dw [N,K], db [N] (None if not wanted).  `into` = (dw_buffer, db_buffer or None): accumulate."""
    bf = _chk_act(dy, x2d)
    M, N = dy.shape
    K = x2d.shape[1]
    eng = _abi_engine(engine)
    if into is not None:
        dw, db = into
        _chk(dw, db)
        if dw.numel() != N * K or (db is not None and db.numel() != N):
            raise ValueError("gradient buffer of the wrong size")
        if not want_bias:
            db = None
        acc = 1
    else:
        dw = torch.empty(N, K, dtype=torch.float32, device=dy.device)
        db = torch.empty(N, dtype=torch.float32, device=dy.device) if want_bias else None
        acc = 0
    if bf:
        nb = _L().pa2d_gemm_bwd_weight_workspace_bf16(M, N, K)
        ws = _ws(nb, dy)
        _lib.check(_L().pa2d_gemm_bwd_weight_bf16(_p(dy), N, _p(x2d), K, _p(dw), _p(db), ws.data_ptr(), nb, M, N, K, acc,
                                                  _stream()), "gemm_bwd_weight_bf16")
        return dw, db
    nb = _L().pa2d_gemm_bwd_weight_workspace(M, N, K, eng)
    ws = _ws(nb, dy)
    _lib.check(_L().pa2d_gemm_bwd_weight(_p(dy), N, _p(x2d), K, _p(dw), _p(db), ws.data_ptr(), nb, M, N, K, acc, eng,
                                         _stream()), "gemm_bwd_weight")
    return dw, db


# ---------------------------------------------------------------------------------------------- weights_frozen()
class _FrozenScope:
    """Book-keeping of one `weights_frozen()` scope: ONE table of everything derived from a weight inside it (conv packs,
    GEMM weight images, the fused tail's images), key -> (kept tensors, buffer, remake).  The key is the kind ("pack",
    "pack1", "image"), the weights' addresses and all the layout depends on: the dims (with the depth of a 3-D mesh, None for
    the 3x3 conv: a 2-D and a 3-D model in one scope never share a pack), the direction and the engine (so models on different
    engines can share a scope).  The kept tensors are those weights (their addresses stay theirs); remake() derives the
    buffer again, in place."""

    def __init__(self):
        self.table = {}

    def refresh(self):
        """Re-make every entry in place (same device pointers): called before replaying a hipGraph that was captured
        inside this scope, so the graph's launches always see the current weights."""
        for _, _, remake in self.table.values():
            remake()

    def _view(self, kind):
        return MappingProxyType({k[1:]: keep + (buf,) for k, (keep, buf, _) in self.table.items() if k[0] == kind})

    # read-only views of the table, one per kind: the key without the kind -> (weights..., buffer)
    packs = property(lambda self: self._view("pack"))      # (wx ptr, wf ptr, B, H, W, depth, C, direction, engine) -> (wx, wf, pack)
    packs1 = property(lambda self: self._view("pack1"))    # single 3x3 conv: (w ptr, B, H, W, C, direction, engine) -> (w, pack)
    images = property(lambda self: self._view("image"))    # (w ptr, transposed, N, K, engine) -> (w, image) of the row-stationary
    #                                                        linear; transposed = "tail": the fused block tail's image of w


_frozen = []      # stack of active scopes; None: an `unscoped()` frame


class weights_frozen:
    """Context manager declaring that no parameter changes inside it (the model calls + backward of one training
    iteration, a rollout).  Inside, the K-major pack of each layer's conv weights is built on first use and
    reused by later calls; outside a scope every conv call packs its weights itself (always correct, whatever
    changed the weights).  `with weights_frozen() as scope:` exposes `scope.refresh()`; `weights_frozen(scope)` enters that
    scope again, with the entries it already holds."""

    def __init__(self, scope=None):
        self.scope = scope

    def __enter__(self):
        _frozen.append(_FrozenScope() if self.scope is None else self.scope)
        return _frozen[-1]

    def __exit__(self, *exc):
        _frozen.pop()
        return False


class unscoped:
    """Context manager under which every op behaves as outside any scope (a null frame on the stack): for calls on a
    temporary weight (a concatenation, a scaled copy), which a scope would keep alive and re-make without ever hitting it."""

    def __enter__(self):
        _frozen.append(None)

    def __exit__(self, *exc):
        _frozen.pop()
        return False


def _active():
    """The scope that `_scoped` fills, or None (no scope, or under `unscoped()`)."""
    return _frozen[-1] if _frozen else None


def _scoped(key, nbytes, make, keep, *args):
    """Device pointer of the buffer that `make(buffer, *args)` fills from the weights `keep`: made once per `key` in the
    active scope and re-made by its refresh().  0 without a scope, or where the buffer has no bytes: the call then derives it
    in its own workspace.  nbytes: a number, or a function that is asked for it only when the buffer has to be made."""
    scope = _active()
    if scope is None or nbytes == 0:
        return 0
    hit = scope.table.get(key)
    if hit is None:
        buf = torch.empty(nbytes() if callable(nbytes) else nbytes, dtype=torch.uint8, device=keep[0].device)
        make(buf, *args)
        hit = scope.table[key] = (keep, buf, lambda: make(buf, *args))
    return hit[1].data_ptr()


# ---------------------------------------------------------------------------------------------- convs
class _Conv(NamedTuple):
    """One family of conv entry points of the C ABI, by the names of its symbols."""
    nw: int             # weights per call: 1 (the single conv) or 2 (the x / fx pair, output [.., 2C])
    depth: bool         # dims are (B, H, W, depth, C): the 3x3x3 conv of a [B, H, W, depth] mesh
    bf16: bool          # has *_bf16 twins for bf16 storage (no engine argument; the bf16 kernels' pack layout, no dims)
    planes: bool        # the operands arrive as bf16 plane images; the bias gradients are made elsewhere
    pack_bytes: str
    pack: str
    fwd: str
    bwd: str
    fwd_ws: str         # workspace query of the forward (from planes: one pack) ...
    bwd_ws: str         # ... and of the backward


def _conv_kind(stem, nw, depth=False, bf16=False, planes=False):
    p, sfx = "pa2d_" + stem, "_planes" if planes else ""
    return _Conv(nw, depth, bf16, planes, p + "_pack_bytes", p + "_pack", p + "_fwd" + sfx, p + "_bwd" + sfx,
                 p + ("_pack_bytes" if planes else "_fwd_workspace"), p + "_workspace" + sfx)


_PAIR = _conv_kind("conv3x3x2", 2, bf16=True)
_SINGLE = _conv_kind("conv3x3", 1)        # in_project_x of the conv slice predictors: one Conv2d(C, C, 3, 1, 1), fp32 storage only
_PAIR3D = _conv_kind("conv3x3x3x2", 2, depth=True)
_PLANES = _conv_kind("conv3x3x2", 2, planes=True)      # shares the packs of _PAIR


def _make_pack(pack, kind, weights, dims, direction, eng, b16):
    name = kind.pack + "_bf16" if b16 else kind.pack
    tail = (dims[-1], direction) if b16 else dims + (direction, eng)
    _lib.check(getattr(_L(), name)(*[_p(w) for w in weights], pack.data_ptr(), pack.numel(), *tail, _stream()), name[5:])


def _conv_pack(kind, weights, dims, direction, eng, b16):
    """Pack pointer for the active scope (0 = let the conv call pack into its workspace).  b16: the pack of the
    bf16-storage entry points (eng is ENGINE_BF16S then)."""
    if _active() is None:
        return 0
    if kind.nw == 1:
        key = ("pack1", weights[0].data_ptr()) + dims + (direction, eng)
    else:
        key = ("pack", weights[0].data_ptr(), weights[1].data_ptr()) + dims[:3] + (dims[3] if kind.depth else None, dims[-1],
                                                                                   direction, eng)
    return _scoped(key, lambda: getattr(_L(), kind.pack_bytes)(dims[-1]), _make_pack, weights, kind, weights, dims, direction,
                   eng, b16)


def _conv_fwd(kind, x, wb, N, dims, eng):
    """The forward of every conv kind: x [B, N, C] (or its plane image), wb = (w, b) per weight, dims = (B, H, W[, depth],
    C), eng as resolved by the wrapper.  Returns [B, N, nw * C] of x's storage type (fp32 from planes)."""
    L, Cc, b16 = _L(), dims[-1], kind.bf16 and eng == ENGINE_BF16S
    sfx, eargs = ("_bf16", ()) if b16 else ("", (eng,))
    out = torch.empty(dims[0], N, kind.nw * Cc, dtype=torch.float32 if kind.planes else x.dtype, device=x.device)
    pre = _conv_pack(kind, wb[::2], dims, 0, eng, b16)
    e0, e1 = _events("conv")
    nb = getattr(L, kind.fwd_ws + sfx)(*((Cc,) if kind.planes else dims + eargs))
    ws = _ws(nb, x)
    name = kind.fwd + sfx
    _lib.check(getattr(L, name)(_p(x), *[_p(t) for t in wb], _p(out), pre, ws.data_ptr(), nb, *dims, *eargs, _stream(), e0, e1),
               name[5:])
    return out


def _conv_bwd(kind, dout, x, weights, N, dims, eng, need_dx, into):
    """The backward of every conv kind: returns (dx [B, N, C] or None, then per weight dw, db — dw only from planes);
    `into`: those parameter gradients' buffers, to accumulate into."""
    L, Cc, b16 = _L(), dims[-1], kind.bf16 and eng == ENGINE_BF16S
    sfx, eargs = ("_bf16", ()) if b16 else ("", (eng,))
    dx = torch.empty(dims[0], N, Cc, dtype=torch.float32 if kind.planes else x.dtype, device=x.device) if need_dx else None
    shapes = [w.shape for w in weights] if kind.planes else [s for w in weights for s in (w.shape, (Cc,))]
    grads, acc = _grad_outputs(into, shapes, x)
    pre = _conv_pack(kind, weights, dims, 1, eng, b16) if need_dx else 0
    e0, e1 = _events("conv") if need_dx else (0, 0)
    nb = getattr(L, kind.bwd_ws + sfx)(*dims, *eargs)
    ws = _ws(nb, x)
    name = kind.bwd + sfx
    _lib.check(getattr(L, name)(_p(dout), _p(x), *[_p(w) for w in weights], _p(dx), *[_p(g) for g in grads], pre,
                                ws.data_ptr(), nb, *dims, acc, *eargs, _stream(), e0, e1), name[5:])
    return (dx,) + grads


def conv3x3x2_fwd(xn, wx, bx, wf, bf, H, W, engine=None):
    """xn [B,N,C] -> [B,N,2C] = [x_mid | fx_mid]."""
    _chk(wx, bx, wf, bf)
    eng = ENGINE_BF16S if _chk_act(xn) else _abi_engine(engine)
    B, N, Cc = xn.shape
    return _conv_fwd(_PAIR, xn, (wx, bx, wf, bf), N, (B, H, W, Cc), eng)


def conv3x3x2_bwd(dout, xn, wx, wf, H, W, need_dx=True, engine=None, into=None):
    """Returns (dxn, dwx, dbx, dwf, dbf); `into` = (dwx, dbx, dwf, dbf) buffers to accumulate into."""
    _chk(wx, wf)
    eng = ENGINE_BF16S if _chk_act(dout, xn) else _abi_engine(engine)
    B, N, Cc = xn.shape
    return _conv_bwd(_PAIR, dout, xn, (wx, wf), N, (B, H, W, Cc), eng, need_dx, into)


def _conv1_engine(engine, *acts):
    _chk(*acts)
    if resolve_engine(engine) == ENGINE_BF16S:
        raise ValueError("the single 3x3 conv has no bf16-storage variant; use the f32, split or bf16 engine")
    return _abi_engine(engine)


def conv3x3_fwd(xn, w, b, H, W, engine=None):
    """xn [B,N,C] -> conv3x3(xn) + b, [B,N,C] (NHWC, zero padding 1)."""
    eng = _conv1_engine(engine, xn, w, b)
    B, N, Cc = xn.shape
    if N != H * W or tuple(w.shape) != (Cc, Cc, 3, 3):
        raise ValueError(f"need xn [B, H*W, C] and w [C, C, 3, 3]; got {tuple(xn.shape)}, {tuple(w.shape)}, H*W = {H * W}")
    return _conv_fwd(_SINGLE, xn, (w, b), N, (B, H, W, Cc), eng)


def conv3x3_bwd(dout, xn, w, H, W, need_dx=True, engine=None, into=None):
    """Returns (dxn, dw, db); `into` = (dw, db) buffers to accumulate into."""
    eng = _conv1_engine(engine, dout, xn, w)
    B, N, Cc = xn.shape
    if N != H * W or dout.shape != xn.shape:
        raise ValueError(f"need xn, dout [B, H*W, C]; got {tuple(xn.shape)}, {tuple(dout.shape)}")
    return _conv_bwd(_SINGLE, dout, xn, (w,), N, (B, H, W, Cc), eng, need_dx, into)


def _conv3d_engine(engine, *acts):
    """fp32-I/O ABI engine of the 3x3x3 conv; bf16 storage has no 3-D kernels and is refused, never converted."""
    if _chk_act(*acts) or resolve_engine(engine) == ENGINE_BF16S:
        raise NotImplementedError("bf16 storage (engine 'bf16s') is not implemented for the 3-D structured mesh")
    return _abi_engine(engine)


def conv3x3x3x2_fwd(xn, wx, bx, wf, bf, H, W, depth, engine=None):
    """The two Conv3d(C, C, 3, 1, 1) projections of the 3-D structured mesh: xn [B, N = H*W*depth, C] (point
    n = (h*W + w)*depth + d) -> [B, N, 2C] = [x_mid | fx_mid]; weights [C, C, 3, 3, 3]."""
    _chk(wx, bx, wf, bf)
    eng = _conv3d_engine(engine, xn)
    B, N, Cc = xn.shape
    if N != H * W * depth:
        raise ValueError(f"conv3x3x3x2_fwd: N = {N} is not H*W*depth = {H}*{W}*{depth}")
    return _conv_fwd(_PAIR3D, xn, (wx, bx, wf, bf), N, (B, H, W, depth, Cc), eng)


def conv3x3x3x2_bwd(dout, xn, wx, wf, H, W, depth, need_dx=True, engine=None, into=None):
    """Backward of conv3x3x3x2_fwd: returns (dxn, dwx, dbx, dwf, dbf); `into` = (dwx, dbx, dwf, dbf) buffers to
    accumulate into."""
    _chk(wx, wf)
    eng = _conv3d_engine(engine, dout, xn)
    B, N, Cc = xn.shape
    if N != H * W * depth:
        raise ValueError(f"conv3x3x3x2_bwd: N = {N} is not H*W*depth = {H}*{W}*{depth}")
    return _conv_bwd(_PAIR3D, dout, xn, (wx, wf), N, (B, H, W, depth, Cc), eng, need_dx, into)


# ---------------------------------------------------------------------------------------------- operand planes
def conv_planes_mask(B, H, W, Cc, engine):
    """7 when `engine` consumes every conv operand at this shape as bf16 planes (then LayerNorm / slice backward can emit
    the planes directly: layernorm_fwd_planes, slice_bwd_points_planes, conv3x3x2_fwd/bwd_planes)."""
    eng = _abi_engine(engine)
    return _L().pa2d_conv3x3x2_planes_mask(B, H, W, Cc, eng) if eng in (ENGINE_SPLIT, ENGINE_BF16) else 0


def _planes(rows, Cc, eng, like):
    return torch.empty(_L().pa2d_planes_bytes(rows, Cc, eng), dtype=torch.uint8, device=like.device)


def layernorm_fwd_planes(x2d, gamma, beta, engine, eps=LN_EPS):
    """LayerNorm whose output exists ONLY as the bf16 plane image the conv GEMMs stage.  Returns (planes, mean, rstd)."""
    _chk(x2d, gamma, beta)
    rows, Cc = x2d.shape
    eng = _abi_engine(engine)
    planes = _planes(rows, Cc, eng, x2d)
    mean = torch.empty(rows, dtype=torch.float32, device=x2d.device)
    rstd = torch.empty_like(mean)
    _lib.check(_L().pa2d_layernorm_fwd_planes(_p(x2d), _p(gamma), _p(beta), planes.data_ptr(), _p(mean), _p(rstd), rows,
                                              Cc, eps, eng, _stream()), "layernorm_fwd_planes")
    return planes, mean, rstd


def conv3x3x2_fwd_planes(xn_planes, wx, bx, wf, bf, B, H, W, engine):
    """[x_mid | fx_mid] [B, H*W, 2C] fp32 from the plane image of the LayerNorm output."""
    _chk(wx, bx, wf, bf)
    return _conv_fwd(_PLANES, xn_planes, (wx, bx, wf, bf), H * W, (B, H, W, wx.shape[0]), _abi_engine(engine))


def conv3x3x2_bwd_planes(dout_planes, xn_planes, wx, wf, B, H, W, engine, need_dx=True, into=None):
    """(dxn, dwx, dwf) from plane images of dOut and X; `into` = (dwx, dwf) buffers to accumulate into."""
    _chk(wx, wf)
    return _conv_bwd(_PLANES, dout_planes, xn_planes, (wx, wf), H * W, (B, H, W, wx.shape[0]), _abi_engine(engine), need_dx, into)


def slice_bwd_points_planes(xf, dy, ws_w, bs, temperature, o, ds, dn, nrm, B, N, heads, D, M, engine, clamp=True, into=None):
    """slice_bwd_points whose [dX | dF] leaves only as the plane image for the conv backward; also returns the conv bias
    gradients (`nrm` = the forward's slice norms [B*heads, M], from token_attn_fwd).
    Returns (dxf_planes, dbx, dbf, dws, dbs, dtemperature); `into` = (dbx, dbf, dws, dbs, dtemperature)."""
    _chk(xf, dy, ws_w, bs, temperature, o, ds, dn, nrm)
    Cc = heads * D
    eng = _abi_engine(engine)
    planes = _planes(B * N, 2 * Cc, eng, xf)
    (dbx, dbf, dws, dbs, dtemp), acc = _grad_outputs(into, ((Cc,), (Cc,), ws_w.shape, bs.shape, (heads,)), xf)
    nb = _L().pa2d_slice_bwd_workspace(B, N, heads, D, M)
    ws = _ws(nb, xf)
    e0, e1 = _events("slice_bwd")
    _lib.check(_L().pa2d_slice_bwd_points_planes(_p(xf), 2 * Cc, _p(xf, Cc), 2 * Cc, _p(dy), Cc, _p(ws_w), _p(bs),
                                                 _p(temperature), _p(o), _p(ds), _p(dn), _p(nrm), planes.data_ptr(), _p(dbx), _p(dbf),
                                                 _p(dws), _p(dbs), _p(dtemp), ws.data_ptr(), nb, B, N, heads, D, M,
                                                 int(clamp), acc, eng, _stream(), e0, e1), "slice_bwd_points_planes")
    return planes, dbx, dbf, dws, dbs, dtemp


def slice_nchunk(B, N, heads):
    return _L().pa2d_slice_nchunk(B, N, heads)


def _slice_engine_args(engine, bf):
    """The slice entry points of fp32 storage take the engine (exact-fp32 MFMA kernels vs bf16 splits); bf16 storage has none."""
    return () if bf else (_abi_engine(engine),)


def slice_scatter(xm, ldx, xm_off, v, ldv, v_off, ws_w, bs, temperature, B, N, heads, D, M, want_norm=True,
                  clamp=True, engine=None):
    """Partial sums of W^T V per point chunk.  xm / v are base tensors; *_off are float offsets."""
    _chk(ws_w, bs, temperature)
    bf = _chk_act(xm, v)
    nchunk = slice_nchunk(B, N, heads)
    spart = torch.empty(B * heads, nchunk, M, D, dtype=torch.float32, device=xm.device)
    npart = torch.empty(B * heads, nchunk, M, dtype=torch.float32, device=xm.device) if want_norm else None
    e0, e1 = _events("slice_scatter")
    _lib.check(_fn("pa2d_slice_scatter", bf)(_p(xm, xm_off), ldx, _p(v, v_off), ldv, _p(ws_w), _p(bs), _p(temperature),
                                       _p(spart), _p(npart), B, N, heads, D, M, int(clamp), *_slice_engine_args(engine, bf),
                                       _stream(), e0, e1),
               "slice_scatter")
    return spart, npart


def token_attn_fwd(spart, npart, wq, wk, wv, drop=None):
    """`drop` = (thresh, scale, seed, offset): dropout on the attention matrix, a draw of BH*M*M elements."""
    _chk(spart, npart, wq, wk, wv)
    BH, nchunk, M, D = spart.shape
    s = torch.empty(BH, M, D, dtype=torch.float32, device=spart.device)
    nrm = torch.empty(BH, M, dtype=torch.float32, device=spart.device)
    o = torch.empty_like(s)
    args = (_p(spart), _p(npart), _p(wq), _p(wk), _p(wv), _p(s), _p(nrm), _p(o), BH, nchunk, M, D)
    if drop is None:
        _lib.check(_L().pa2d_token_attn_fwd(*args, _stream()), "token_attn_fwd")
    else:
        _lib.check(_L().pa2d_token_attn_fwd_dropout(*args, *_drop_args(drop), _stream()), "token_attn_fwd_dropout")
    return s, nrm, o


def token_attn_bwd(s, nrm, wq, wk, wv, dopart, into=None, drop=None):
    """`drop`: the forward's draw; the kernel makes the mask again."""
    _chk(s, nrm, wq, wk, wv, dopart)
    BH, nchunk, M, D = dopart.shape
    ds = torch.empty_like(s)
    dn = torch.empty_like(nrm)
    (dwq, dwk, dwv), acc = _grad_outputs(into, ((D, D), (D, D), (D, D)), s)
    nb = _L().pa2d_token_attn_bwd_workspace(BH, D)
    ws = _ws(nb, s)
    args = (_p(s), _p(nrm), _p(wq), _p(wk), _p(wv), _p(dopart), _p(ds), _p(dn), _p(dwq), _p(dwk), _p(dwv), ws.data_ptr(), nb,
            BH, nchunk, M, D, acc)
    if drop is None:
        _lib.check(_L().pa2d_token_attn_bwd(*args, _stream()), "token_attn_bwd")
    else:
        _lib.check(_L().pa2d_token_attn_bwd_dropout(*args, *_drop_args(drop), _stream()), "token_attn_bwd_dropout")
    return ds, dn, dwq, dwk, dwv


# ---------------------------------------------------------------------------------------------- training-mode dropout
# Masks are never stored: a DRAW (seed, offset, n) names them (include/pa2d.h), the kernels evaluate Philox4x32-10 for it,
# forward and backward alike.  The package keeps one generator: a 64-bit seed and the offset of the next draw.
DROPOUT_TRIP = 2048 * 256 * 4        # elements one grid-stride trip of dropout_residual covers (PA2D_DROPOUT_TRIP)
_MASK64 = (1 << 64) - 1
_dropout = {"seed": None, "offset": 0, "torch_seed": None}


def dropout_constants(p):
    """(thresh, scale) the kernels take for dropout probability p: floor(p 2^32) and fp32(1 / (1 - p)).  Host arithmetic."""
    p = float(p)
    if p == 1.0:
        raise ValueError("dropout p = 1 drops everything and has no finite scale 1 / (1 - p)")
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout probability has to be in [0, 1); got {p}")
    return int(p * 4294967296.0), float(torch.tensor(1.0 / (1.0 - p), dtype=torch.float64).to(torch.float32))


def _dropout_latch():
    """Without an explicit seed the generator follows torch's: it takes torch.initial_seed() at first use and again, with
    offset 0, whenever that value has changed since (torch.manual_seed(s) with a new s; an explicit seed is dropped then)."""
    ts = torch.initial_seed()
    if _dropout["seed"] is None or ts != _dropout["torch_seed"]:
        _dropout.update(seed=ts & _MASK64, offset=0, torch_seed=ts)


def dropout_manual_seed(seed):
    """Seed the package's dropout generator; the next draw starts at offset 0."""
    _dropout.update(seed=int(seed) & _MASK64, offset=0, torch_seed=torch.initial_seed())


def dropout_state():
    """(seed, offset) of the next draw."""
    _dropout_latch()
    return _dropout["seed"], _dropout["offset"]


def dropout_reserve(n):
    """(seed, offset) of a draw of n elements; the generator moves on by the ceil(n / 4) counters the draw uses."""
    _dropout_latch()
    draw = (_dropout["seed"], _dropout["offset"])
    _dropout["offset"] = (_dropout["offset"] + (int(n) + 3) // 4) & _MASK64
    return draw


def dropout_keep_host(seed, offset, first, count, thresh):
    """uint8 [count] host tensor: 1 where element first + i of the draw (seed, offset) is kept.  Host code, no GPU."""
    keep = torch.empty(int(count), dtype=torch.uint8)
    _lib.check(_L().pa2d_dropout_keep_host(int(seed) & _MASK64, int(offset) & _MASK64, int(first), int(count), int(thresh),
                                           keep.data_ptr()), "dropout_keep_host")
    return keep


def _drop_args(drop):
    thresh, scale, seed, offset = drop
    if not 0 <= int(thresh) < (1 << 32):
        raise ValueError(f"dropout threshold {thresh} is not a 32-bit word")
    return int(thresh), float(scale), int(seed) & _MASK64, int(offset) & _MASK64


def dropout_residual(z, res, drop):
    """out = (res or 0) + keep * z * scale over the flat tensor (element index = flat index of z); `drop` = (thresh, scale,
    seed, offset).  z and res may be views at any 4-byte aligned address (the kernel then goes element by element)."""
    for t in (z, res):
        if t is not None and (not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous()):
            raise ValueError("dropout_residual needs contiguous fp32 tensors on the GPU")
    if res is not None and res.numel() != z.numel():
        raise ValueError("dropout_residual: z and res differ in size")
    out = torch.empty_like(z)
    _lib.check(_L().pa2d_dropout_residual(_p(z), _p(res), _p(out), z.numel(), *_drop_args(drop), _stream()),
               "dropout_residual")
    return out


def deslice_fwd(xm, ldx, xm_off, o, ws_w, bs, temperature, B, N, heads, D, M, clamp=True, engine=None):
    _chk(o, ws_w, bs, temperature)
    bf = _chk_act(xm)
    y = torch.empty(B, N, heads * D, dtype=xm.dtype, device=xm.device)
    e0, e1 = _events("deslice")
    _lib.check(_fn("pa2d_deslice_fwd", bf)(_p(xm, xm_off), ldx, _p(o), _p(ws_w), _p(bs), _p(temperature), _p(y), heads * D,
                                     B, N, heads, D, M, int(clamp), *_slice_engine_args(engine, bf), _stream(), e0, e1),
               "deslice_fwd")
    return y


# ---------------------------------------------------------------------------------------------- fused block tail
def block_tail_supported(Cc, heads, D, M, hidden, act, engine=None):
    """True where `block_tail_fwd` runs (include/pa2d.h: pa2d_block_tail_supported); a host-side query, no GPU needed.
    bf16 storage has no fused tail."""
    eng = resolve_engine(engine)
    if eng == ENGINE_BF16S or act not in ACT_IDS:
        return False
    return bool(_L().pa2d_block_tail_supported(Cc, heads, D, M, hidden, ACT_IDS[act], eng))


def _make_tail_image(img, w, N, K, eng):
    _lib.check(_L().pa2d_block_tail_weight_image(_p(w), w.shape[1], img.data_ptr(), img.numel(), N, K, eng, _stream()),
               "block_tail_weight_image")


def block_tail_fwd(xm, ldx, xm_off, o, ws_w, bs, temperature, fx2d, wo, bo, g2, be2, w1, b1, w2, b2, gn, bn, B, N, heads,
                   D, M, act, clamp=True, engine=None, debug=False, eps=LN_EPS):
    """The row-local tail of a block in ONE launch (no-grad forwards): de-slice, to_out + residual `fx2d`, ln_2, the MLP
    and its residual, and — when gn / bn are given — the LayerNorm that follows (the next block's ln_1, or ln_3).
    Returns (out [B*N, C], xn [B*N, C] or None, debug), debug = (y, a, h) copies of the stages when asked for."""
    _chk(o, ws_w, bs, temperature, fx2d, wo, bo, g2, be2, w1, b1, w2, b2, gn, bn)
    if _chk_act(xm):
        raise TypeError("the fused block tail has no bf16-storage variant")
    eng = _abi_engine(engine)
    Cc, hidden, rows = heads * D, w1.shape[0], B * N
    if tuple(wo.shape) != (Cc, Cc) or tuple(w1.shape) != (hidden, Cc) or tuple(w2.shape) != (Cc, hidden):
        raise ValueError("block_tail_fwd: weight shapes do not match heads * D and the hidden width")
    if tuple(fx2d.shape) != (rows, Cc) or (gn is None) != (bn is None):
        raise ValueError("block_tail_fwd: fx must be [B*N, C]; gn and bn go together")
    dev = xm.device
    out = torch.empty(rows, Cc, dtype=torch.float32, device=dev)
    xn = torch.empty(rows, Cc, dtype=torch.float32, device=dev) if gn is not None else None
    dbg = None
    if debug:
        dbg = (torch.empty(rows, Cc, dtype=torch.float32, device=dev), torch.empty(rows, Cc, dtype=torch.float32, device=dev),
               torch.empty(rows, hidden, dtype=torch.float32, device=dev))
    y_d, a_d, h_d = dbg if dbg is not None else (None, None, None)
    imgs = (0, 0, 0)
    if _L().pa2d_block_tail_supported(Cc, heads, D, M, hidden, ACT_IDS[act], eng):
        def image(w):      # inside weights_frozen(): made once per weight, re-made by scope.refresh()
            N, K = w.shape
            return _scoped(("image", w.data_ptr(), "tail", N, K, eng), lambda: _L().pa2d_block_tail_image_bytes(N, K),
                           _make_tail_image, (w,), w, N, K, eng)
        imgs = tuple(image(w) for w in (wo, w1, w2))
    nb = 0 if all(imgs) else _L().pa2d_block_tail_workspace(Cc, hidden)
    ws = _ws(nb, xm) if nb else None
    _lib.check(_L().pa2d_block_tail_fwd(_p(xm, xm_off), ldx, _p(o), _p(ws_w), _p(bs), _p(temperature), _p(fx2d), Cc, _p(wo),
                                        _p(bo), _p(g2), _p(be2), _p(w1), _p(b1), _p(w2), _p(b2), _p(gn), _p(bn), _p(out),
                                        _p(xn), _p(y_d), _p(a_d), _p(h_d), *imgs, _p(ws), nb, B, N, heads, D, M, hidden,
                                        ACT_IDS[act], int(clamp), eng, eps, _stream()), "block_tail_fwd")
    return out, xn, dbg


def slice_bwd_points(xf, dy, ws_w, bs, temperature, o, ds, dn, B, N, heads, D, M, clamp=True, into=None, engine=None):
    """xf = [B,N,2C] ([x_mid | fx_mid]); returns dxf [B,N,2C], dws, dbs, dtemperature [heads]."""
    _chk(ws_w, bs, temperature, o, ds, dn)
    bf = _chk_act(xf, dy)
    Cc = heads * D
    dxf = torch.empty_like(xf)
    (dws, dbs, dtemp), acc = _grad_outputs(into, (ws_w.shape, bs.shape, (heads,)), xf)
    nb = _L().pa2d_slice_bwd_workspace(B, N, heads, D, M)
    ws = _ws(nb, xf)
    e0, e1 = _events("slice_bwd")
    _lib.check(_fn("pa2d_slice_bwd_points", bf)(_p(xf), 2 * Cc, _p(xf, Cc), 2 * Cc, _p(dy), Cc, _p(ws_w), _p(bs),
                                          _p(temperature), _p(o), _p(ds), _p(dn), _p(dxf), 2 * Cc, _p(dxf, Cc),
                                          2 * Cc, _p(dws), _p(dbs), _p(dtemp), ws.data_ptr(), nb, B, N, heads, D, M,
                                          int(clamp), acc, *_slice_engine_args(engine, bf), _stream(), e0, e1),
               "slice_bwd_points")
    return dxf, dws, dbs, dtemp


# ---------------------------------------------------------------------------------------------- auto-encoder attention
# Materialised slice weights and the de-slice with explicit weights (pa2d_slice_weights_* / pa2d_deslice_weights_*): exact
# fp32 on every engine, so these take no `engine`.
def _row_view(x, heads, D):
    """(pitch, B, N) of an fp32 [B, N, >= heads*D] activation whose rows may be strided (a column view of the conv
    output): unit stride along the features, rows at a constant pitch."""
    if not x.is_cuda:
        raise RuntimeError("libpa2d ops need tensors on the GPU (no CPU fallback exists in this package)")
    if x.dtype != torch.float32:
        raise TypeError(f"libpa2d ops are fp32; got {x.dtype}")
    B, N, Cx = x.shape
    if Cx < heads * D or x.stride(2) != 1 or (B > 1 and x.stride(0) != N * x.stride(1)):
        raise ValueError("need rows of unit feature stride at one constant pitch")
    return x.stride(1), B, N


def slice_weights_fwd(xm, ws_w, bs, temperature, heads, clamp=True):
    """xm [B, N, >= C] (x_mid; rows may be strided); returns the softmax slice weights sw [B, heads, N, M]."""
    _chk(ws_w, bs, temperature)
    M, D = ws_w.shape
    ldx, B, N = _row_view(xm, heads, D)
    sw = torch.empty(B, heads, N, M, dtype=torch.float32, device=xm.device)
    e0, e1 = _events("slice_weights")
    _lib.check(_L().pa2d_slice_weights_fwd(_p(xm), ldx, _p(ws_w), _p(bs), _p(temperature), _p(sw), B, N, heads, D, M,
                                           int(clamp), _stream(), e0, e1), "slice_weights_fwd")
    return sw


def slice_weights_bwd(xm, ws_w, bs, temperature, dsw, clamp=True, need_dx=True, into=None):
    """Returns dxm [B, N, C] (None without need_dx), dws [M, D], dbs [M], dtemperature [heads]."""
    _chk(ws_w, bs, temperature, dsw)
    M, D = ws_w.shape
    heads = temperature.numel()
    ldx, B, N = _row_view(xm, heads, D)
    if tuple(dsw.shape) != (B, heads, N, M):
        raise ValueError(f"dsw must be [B, heads, N, M] = {(B, heads, N, M)}; got {tuple(dsw.shape)}")
    dxm = torch.empty(B, N, heads * D, dtype=torch.float32, device=xm.device) if need_dx else None
    (dws, dbs, dtemp), acc = _grad_outputs(into, (ws_w.shape, bs.shape, (heads,)), dsw)
    nb = _L().pa2d_slice_weights_bwd_workspace(B, N, heads, D, M)
    ws = _ws(nb, dsw)
    e0, e1 = _events("slice_weights_bwd")
    _lib.check(_L().pa2d_slice_weights_bwd(_p(xm), ldx, _p(ws_w), _p(bs), _p(temperature), _p(dsw), _p(dxm), heads * D,
                                           _p(dws), _p(dbs), _p(dtemp), ws.data_ptr(), nb, B, N, heads, D, M, int(clamp),
                                           acc, _stream(), e0, e1), "slice_weights_bwd")
    return dxm, dws, dbs, dtemp


def deslice_weights_fwd(code, w):
    """code [B, heads, M, D], w [B, heads, N, M] -> y [B, N, heads*D] (einsum "bhgc,bhng->bhnc" + rearrange)."""
    _chk(code, w)
    B, heads, M, D = code.shape
    N = w.shape[2]
    if tuple(w.shape) != (B, heads, N, M):
        raise ValueError(f"slice weights must be [B, heads, N, M] = {(B, heads, N, M)}; got {tuple(w.shape)}")
    y = torch.empty(B, N, heads * D, dtype=torch.float32, device=code.device)
    e0, e1 = _events("deslice_weights")
    _lib.check(_L().pa2d_deslice_weights_fwd(_p(code), _p(w), _p(y), heads * D, B, N, heads, D, M, _stream(), e0, e1),
               "deslice_weights_fwd")
    return y


def deslice_weights_bwd(code, w, dy, need_dcode=True, need_dw=True):
    """Returns (dcode [B, heads, M, D] or None, dw [B, heads, N, M] or None)."""
    _chk(code, w, dy)
    B, heads, M, D = code.shape
    N = w.shape[2]
    dcode = torch.empty_like(code) if need_dcode else None
    dw = torch.empty_like(w) if need_dw else None
    nb = _L().pa2d_deslice_weights_bwd_workspace(B, N, heads, D, M) if need_dcode else 0
    ws = _ws(nb, code) if need_dcode else None
    e0, e1 = _events("deslice_weights_bwd")
    _lib.check(_L().pa2d_deslice_weights_bwd(_p(code), _p(w), _p(dy), heads * D, _p(dcode), _p(dw), _p(ws), nb, B, N,
                                             heads, D, M, _stream(), e0, e1), "deslice_weights_bwd")
    return dcode, dw


# ---------------------------------------------------------------------------------------------- SequenSolver stages
# Sequence attention among the T frame tokens (pa2d_seq_attn_*) and the slice weights predicted from the code and the two
# point coordinates (the P = 2 case of the LearnSlice stage below): exact fp32 on every engine, so these take no `engine`.
SEQ_ATTN_MAX_T, SEQ_ATTN_MAX_DIM = 32, 1024
HEAD_SEQ_ATTN_MAX_T, HEAD_SEQ_ATTN_MAX_SD = 32, 64      # the fused head attention (pa2d_head_seq_attn_*); sd % 4 == 0
CODE_SW_HIDDEN, CODE_SW_DEPTH = 64, 1


def seq_attn_fwd(q, k, v, scale, res=None, causal=False):
    """q, k, v [B, T, dim] -> (out [B, T, dim], attn [B, T, T]) with attn = softmax(q k^T * scale), out = attn v (+ res);
    `causal`: the softmax of row i runs over j <= i, attn[i, j > i] = 0 (pa2d_seq_attn_causal_*)."""
    _chk(q, k, v, res)
    B, T, dim = q.shape
    if k.shape != q.shape or v.shape != q.shape or (res is not None and res.shape != q.shape):
        raise ValueError("q, k, v (and res) must share the shape [B, T, dim]")
    out = torch.empty_like(q)
    attn = torch.empty(B, T, T, dtype=torch.float32, device=q.device)
    fn = _L().pa2d_seq_attn_causal_fwd if causal else _L().pa2d_seq_attn_fwd
    _lib.check(fn(_p(q), _p(k), _p(v), _p(res), _p(out), _p(attn), B, T, dim, float(scale), _stream()), "seq_attn_fwd")
    return out, attn


def seq_attn_bwd(q, k, v, attn, dout, scale, causal=False):
    """Returns (dq, dk, dv), each [B, T, dim]."""
    _chk(q, k, v, attn, dout)
    B, T, dim = q.shape
    if dout.shape != q.shape or tuple(attn.shape) != (B, T, T):
        raise ValueError("dout must be [B, T, dim] and attn [B, T, T]")
    dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
    nb = _L().pa2d_seq_attn_bwd_workspace(B, T)
    ws = _ws(nb, q)
    fn = _L().pa2d_seq_attn_causal_bwd if causal else _L().pa2d_seq_attn_bwd
    _lib.check(fn(_p(q), _p(k), _p(v), _p(attn), _p(dout), _p(dq), _p(dk), _p(dv), ws.data_ptr(), nb, B, T, dim, float(scale),
                  _stream()), "seq_attn_bwd")
    return dq, dk, dv


def seq_attn_causal_fwd(q, k, v, scale, res=None):
    return seq_attn_fwd(q, k, v, scale, res=res, causal=True)


def seq_attn_causal_bwd(q, k, v, attn, dout, scale):
    return seq_attn_bwd(q, k, v, attn, dout, scale, causal=True)


def _head_attn_shapes(x, wq, wk, wv):
    if x.dim() != 3:
        raise ValueError(f"x must be [G, T, sd] (G = B*heads groups); got {tuple(x.shape)}")
    G, T, sd = x.shape
    if any(tuple(w.shape) != (sd, sd) for w in (wq, wk, wv)):
        raise ValueError(f"wq, wk, wv must be [sd, sd] = {(sd, sd)}; got {[tuple(w.shape) for w in (wq, wk, wv)]}")
    return G, T, sd


def head_seq_attn_fwd(x, wq, wk, wv, scale, res=None, causal=True):
    """x [G, T, sd] (the LayerNorm output as G = B*heads groups), wq, wk, wv [sd, sd] -> (out [G, T, sd], attn [G, T, T]):
    projections, (causal) softmax attention and the residual in one launch (pa2d_head_seq_attn_fwd; T <= HEAD_SEQ_ATTN_MAX_T,
    sd % 4 == 0, sd <= HEAD_SEQ_ATTN_MAX_SD)."""
    _chk(x, wq, wk, wv, res)
    G, T, sd = _head_attn_shapes(x, wq, wk, wv)
    if res is not None and res.shape != x.shape:
        raise ValueError("res must have the shape of x")
    out = torch.empty_like(x)
    attn = torch.empty(G, T, T, dtype=torch.float32, device=x.device)
    _lib.check(_L().pa2d_head_seq_attn_fwd(_p(x), _p(wq), _p(wk), _p(wv), _p(res), _p(out), _p(attn), G, T, sd, float(scale),
                                           int(bool(causal)), _stream()), "head_seq_attn_fwd")
    return out, attn


def head_seq_attn_bwd(x, wq, wk, wv, attn, dout, scale, causal=True, into=None):
    """Returns (dx [G, T, sd], dwq, dwk, dwv [sd, sd]); `into` = the three gradient buffers to add into."""
    _chk(x, wq, wk, wv, attn, dout)
    G, T, sd = _head_attn_shapes(x, wq, wk, wv)
    if dout.shape != x.shape or tuple(attn.shape) != (G, T, T):
        raise ValueError("dout must be [G, T, sd] and attn [G, T, T]")
    dx = torch.empty_like(x)
    grads, acc = _grad_outputs(into, (wq.shape, wk.shape, wv.shape), x)
    nb = _L().pa2d_head_seq_attn_bwd_workspace(G, T, sd)
    ws = _ws(nb, x)
    _lib.check(_L().pa2d_head_seq_attn_bwd(_p(x), _p(wq), _p(wk), _p(wv), _p(attn), _p(dout), _p(dx), *(_p(g) for g in grads),
                                           ws.data_ptr(), nb, G, T, sd, float(scale), int(bool(causal)), acc, _stream()),
               "head_seq_attn_bwd")
    return (dx,) + tuple(grads)


def _two_coordinates(code, pos):
    if pos.dim() != 3 or tuple(pos.shape) != (code.shape[0], pos.shape[1], 2):
        raise ValueError(f"positions must be the two point coordinates [B, N, 2]; got {tuple(pos.shape)}")


def code_slice_weights_fwd(code, pos, params):
    """code [B, M, C], pos [B, N, 2], params = (w1, b1, w2, b2, w3, b3) of weight_projection -> sw [B, 1, N, M]: the
    coordinates are P = 2 point features of point_slice_weights_fwd."""
    _two_coordinates(code, pos)
    return point_slice_weights_fwd(code, pos, params)


def code_slice_weights_bwd(code, pos, params, dsw, need_dcode=True, into=None):
    """Returns (dcode [B, M, C] or None, dw1, db1, dw2, db2, dw3, db3); `into` = the six gradient buffers to add into."""
    _two_coordinates(code, pos)
    return point_slice_weights_bwd(code, pos, params, dsw, need_dcode=need_dcode, into=into)


# ---------------------------------------------------------------------------------------------- LearnSlice stages
# The slice weights from the code and P features per point (pa2d_point_slice_weights_*: the point part of the first layer is
# 1 <= P <= 128 wide) and the trainer's loss (pa2d_slice_mse_*).  Exact fp32, no `engine`.
POINT_SW_MAX_P = 128


def _point_sw_shapes(code, feat, params):
    w1, b1, w2, b2, w3, b3 = params
    if code.dim() != 3 or feat.dim() != 3 or feat.shape[0] != code.shape[0]:
        raise ValueError(f"code must be [B, M, C] and the point features [B, N, P]; got {tuple(code.shape)} and "
                         f"{tuple(feat.shape)}")
    B, M, Cc = code.shape
    N, P = feat.shape[1], feat.shape[2]
    hidden = w1.shape[0]
    want = ((hidden, Cc + P), (hidden,), (hidden, hidden), (hidden,), (1, hidden), (1,))
    if tuple(tuple(p.shape) for p in params) != want:
        raise ValueError(f"weight_projection must be MLP(C+P, hidden, 1) with one hidden layer and C+P = {Cc} + {P}: "
                         f"shapes {want}, got {tuple(tuple(p.shape) for p in params)}")
    return B, N, M, Cc, P, hidden


def point_slice_weights_fwd(code, feat, params):
    """code [B, M, C], feat [B, N, P], params = (w1, b1, w2, b2, w3, b3) of weight_projection -> sw [B, 1, N, M]."""
    B, N, M, Cc, P, hidden = _point_sw_shapes(code, feat, params)
    _chk(code, feat, *params)
    sw = torch.empty(B, 1, N, M, dtype=torch.float32, device=code.device)
    e0, e1 = _events("point_slice_weights")
    _lib.check(_L().pa2d_point_slice_weights_fwd(_p(code), _p(feat), *(_p(t) for t in params), _p(sw), B, N, M, Cc, P,
                                                 hidden, CODE_SW_DEPTH, _stream(), e0, e1), "point_slice_weights_fwd")
    return sw


def point_slice_weights_bwd(code, feat, params, dsw, need_dcode=True, into=None):
    """Returns (dcode [B, M, C] or None, dw1, db1, dw2, db2, dw3, db3); `into` = the six gradient buffers to add into."""
    B, N, M, Cc, P, hidden = _point_sw_shapes(code, feat, params)
    if tuple(dsw.shape) != (B, 1, N, M):
        raise ValueError(f"dsw must be [B, 1, N, M] = {(B, 1, N, M)}; got {tuple(dsw.shape)}")
    _chk(code, feat, dsw, *params)
    dcode = torch.empty_like(code) if need_dcode else None
    grads, acc = _grad_outputs(into, tuple(p.shape for p in params), code)
    nb = _L().pa2d_point_slice_weights_bwd_workspace(B, N, M, Cc, P)
    ws = _ws(nb, code)
    e0, e1 = _events("point_slice_weights_bwd")
    _lib.check(_L().pa2d_point_slice_weights_bwd(_p(code), _p(feat), *(_p(t) for t in params), _p(dsw), _p(dcode),
                                                 *(_p(g) for g in grads), ws.data_ptr(), nb, B, N, M, Cc, P, hidden,
                                                 CODE_SW_DEPTH, acc, _stream(), e0, e1), "point_slice_weights_bwd")
    return (dcode,) + tuple(grads)


# ---------------------------------------------------------------------------------------------- conv slice predictors
# z-score over a whole tensor and the wide slice weights (pa2d_zscore_* / pa2d_wide_slice_weights_*): exact fp32 on every
# engine, so these take no `engine`.
def _rows_view(x):
    """(rows, C, pitch) of an fp32 [..., C] activation whose rows sit at one constant pitch (a column view of a wider
    tensor is fine); unit stride along the features."""
    if not x.is_cuda:
        raise RuntimeError("libpa2d ops need tensors on the GPU (no CPU fallback exists in this package)")
    if x.dtype != torch.float32:
        raise TypeError(f"libpa2d ops are fp32; got {x.dtype}")
    Cx = x.shape[-1]
    rows = x.numel() // max(Cx, 1)
    if x.is_contiguous():
        return rows, Cx, Cx
    if x.dim() < 2 or x.stride(-1) != 1:
        raise ValueError("need rows of unit feature stride at one constant pitch")
    pitch = x.stride(-2)
    for d in range(x.dim() - 2, 0, -1):
        if x.shape[d - 1] > 1 and x.stride(d - 1) != x.shape[d] * x.stride(d):
            raise ValueError("need rows of unit feature stride at one constant pitch")
    return rows, Cx, pitch


def zscore_fwd(x):
    """y = (x - x.mean()) / (x.std(unbiased=False) + 1e-8) over ALL elements; returns (y contiguous, stats fp64 [mu, sigma])."""
    rows, Cc, ldx = _rows_view(x)
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    stats = torch.empty(2, dtype=torch.float64, device=x.device)
    nb = _L().pa2d_zscore_workspace(rows, Cc)
    ws = _ws(nb, x)
    _lib.check(_L().pa2d_zscore_fwd(_p(x), ldx, _p(y), _p(stats), ws.data_ptr(), nb, rows, Cc, _stream()), "zscore_fwd")
    return y, stats


def zscore_bwd(dy, y, stats):
    """dx (contiguous) from dy (rows may be strided), the forward's y and statistics."""
    _chk(y)
    rows, Cc, lddy = _rows_view(dy)
    if dy.shape != y.shape or stats.dtype != torch.float64 or stats.numel() != 2:
        raise ValueError("need dy of y's shape and the forward's fp64 statistics")
    dx = torch.empty(y.shape, dtype=torch.float32, device=y.device)
    nb = _L().pa2d_zscore_workspace(rows, Cc)
    ws = _ws(nb, y)
    _lib.check(_L().pa2d_zscore_bwd(_p(dy), lddy, _p(y), _p(stats), _p(dx), Cc, ws.data_ptr(), nb, rows, Cc, _stream()),
               "zscore_bwd")
    return dx


def _group_rows(rows, groups):
    if groups < 1 or rows % groups:
        raise ValueError(f"groups = {groups} must divide the {rows} rows")
    return rows // groups


def zscore_grouped_fwd(x, groups):
    """The z-score of zscore_fwd over `groups` groups of consecutive rows of x [..., C], each with its own statistics, in
    one pair of launches; returns (y contiguous, stats fp64 [groups, 2] = mu, sigma).  Group g equals zscore_fwd on its rows
    alone, bit for bit."""
    rows, Cc, ldx = _rows_view(x)
    rpg = _group_rows(rows, groups)
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    stats = torch.empty(groups, 2, dtype=torch.float64, device=x.device)
    nb = _L().pa2d_zscore_grouped_workspace(groups, rpg, Cc)
    ws = _ws(nb, x)
    _lib.check(_L().pa2d_zscore_grouped_fwd(_p(x), ldx, _p(y), _p(stats), ws.data_ptr(), nb, groups, rpg, Cc, _stream()),
               "zscore_grouped_fwd")
    return y, stats


def zscore_grouped_bwd(dy, y, stats):
    """dx (contiguous) from dy (rows may be strided), the grouped forward's y and statistics [groups, 2]."""
    _chk(y)
    rows, Cc, lddy = _rows_view(dy)
    if dy.shape != y.shape or stats.dtype != torch.float64 or stats.dim() != 2 or stats.shape[1] != 2:
        raise ValueError("need dy of y's shape and the grouped forward's fp64 statistics [groups, 2]")
    groups = stats.shape[0]
    rpg = _group_rows(rows, groups)
    dx = torch.empty(y.shape, dtype=torch.float32, device=y.device)
    nb = _L().pa2d_zscore_grouped_workspace(groups, rpg, Cc)
    ws = _ws(nb, y)
    _lib.check(_L().pa2d_zscore_grouped_bwd(_p(dy), lddy, _p(y), _p(stats), _p(dx), Cc, ws.data_ptr(), nb, groups, rpg, Cc,
                                            _stream()), "zscore_grouped_bwd")
    return dx


def wide_slice_weights_fwd(x, ws_w, bs, temperature, clamp=True):
    """x [..., D] (rows may be strided) -> sw [..., M] = softmax_m((x . ws^T + bs) / t), t = temperature (one scalar)."""
    _chk(ws_w, bs, temperature)
    M, D = ws_w.shape
    rows, Dx, ldx = _rows_view(x)
    if Dx != D or bs.numel() != M or temperature.numel() != 1:
        raise ValueError(f"need x [..., {D}], bs [{M}] and one temperature; got {tuple(x.shape)}, {tuple(bs.shape)}")
    sw = torch.empty(*x.shape[:-1], M, dtype=torch.float32, device=x.device)
    e0, e1 = _events("wide_slice_weights")
    _lib.check(_L().pa2d_wide_slice_weights_fwd(_p(x), ldx, _p(ws_w), _p(bs), _p(temperature), _p(sw), rows, D, M,
                                                int(clamp), _stream(), e0, e1), "wide_slice_weights_fwd")
    return sw


def wide_slice_weights_bwd(x, ws_w, bs, temperature, dsw, clamp=True, need_dx=True, into=None):
    """Returns dx [..., D] (None without need_dx), dws [M, D], dbs [M], dtemperature (temperature's shape)."""
    _chk(ws_w, bs, temperature, dsw)
    M, D = ws_w.shape
    rows, Dx, ldx = _rows_view(x)
    if Dx != D or dsw.numel() != rows * M or temperature.numel() != 1:
        raise ValueError(f"need x [..., {D}] and dsw [..., {M}] over the same rows")
    dx = torch.empty(x.shape, dtype=torch.float32, device=x.device) if need_dx else None
    (dws, dbs, dtemp), acc = _grad_outputs(into, (ws_w.shape, bs.shape, temperature.shape), dsw)
    nb = _L().pa2d_wide_slice_weights_bwd_workspace(rows, D, M)
    ws = _ws(nb, dsw)
    e0, e1 = _events("wide_slice_weights_bwd")
    _lib.check(_L().pa2d_wide_slice_weights_bwd(_p(x), ldx, _p(ws_w), _p(bs), _p(temperature), _p(dsw), _p(dx), D, _p(dws),
                                                _p(dbs), _p(dtemp), ws.data_ptr(), nb, rows, D, M, int(clamp), acc,
                                                _stream(), e0, e1), "wide_slice_weights_bwd")
    return dx, dws, dbs, dtemp


def _slice_mse_shapes(sw, target):
    if sw.dim() < 1 or sw.shape != target.shape:
        raise ValueError(f"sw and target must share a shape [..., M]; got {tuple(sw.shape)} and {tuple(target.shape)}")
    M = sw.shape[-1]
    if M < 1:
        raise ValueError("sw needs at least one slice")
    return sw.numel() // M, M


def slice_mse_fwd(sw, target):
    """sw, target [..., M] -> loss [1] = sum over the rows of mean_m (sw - target)^2."""
    rows, M = _slice_mse_shapes(sw, target)
    _chk(sw, target)
    loss = torch.empty(1, dtype=torch.float32, device=sw.device)
    nb = _L().pa2d_slice_mse_workspace(rows, M)
    ws = _ws(nb, sw)
    _lib.check(_L().pa2d_slice_mse_fwd(_p(sw), _p(target), _p(loss), ws.data_ptr(), nb, rows, M, _stream()), "slice_mse_fwd")
    return loss


def slice_mse_bwd(sw, target, gout):
    """dsw = gout * 2/M * (sw - target); gout: the upstream gradient of the loss, one value on the device."""
    rows, M = _slice_mse_shapes(sw, target)
    if gout.numel() != 1:
        raise ValueError("gout must hold one value")
    _chk(sw, target, gout)
    dsw = torch.empty_like(sw)
    _lib.check(_L().pa2d_slice_mse_bwd(_p(sw), _p(target), _p(gout), _p(dsw), rows, M, _stream()), "slice_mse_bwd")
    return dsw


def head_fwd(xn2d, w, b):
    """y is always fp32 (the model output), whatever the storage type of the activations."""
    _chk(w, b)
    bf = _chk_act(xn2d)
    rows, Cc = xn2d.shape
    O = w.shape[0]
    y = torch.empty(rows, O, dtype=torch.float32, device=xn2d.device)
    _lib.check(_fn("pa2d_head_fwd", bf)(_p(xn2d), _p(w), _p(b), _p(y), rows, Cc, O, _stream()), "head_fwd")
    return y


def head_bwd(dy, xn2d, w, into=None):
    _chk(dy, w)
    bf = _chk_act(xn2d)
    rows, Cc = xn2d.shape
    O = w.shape[0]
    dxn = torch.empty_like(xn2d)
    (dw, db), acc = _grad_outputs(into, (w.shape, (O,)), w)
    nb = _L().pa2d_head_bwd_workspace(rows, Cc, O)
    ws = _ws(nb, dy)
    _lib.check(_fn("pa2d_head_bwd", bf)(_p(dy), _p(xn2d), _p(w), _p(dxn), _p(dw), _p(db), ws.data_ptr(), nb, rows, Cc, O,
                                  acc, _stream()), "head_bwd")
    return dxn, dw, db


def act_bwd(dy, pre, act):
    _chk(dy, pre)
    out = torch.empty_like(dy)
    _lib.check(_L().pa2d_act_bwd(_p(dy), _p(pre), _p(out), dy.numel(), ACT_IDS[act], _stream()), "act_bwd")
    return out


def act_fwd(pre, act):
    _chk(pre)
    out = torch.empty_like(pre)
    _lib.check(_L().pa2d_act_fwd(_p(pre), _p(out), pre.numel(), ACT_IDS[act], _stream()), "act_fwd")
    return out


# ---------------------------------------------------------------------------------------------- SURVEY 8(f)-1
def sumsq(flat):
    _chk(flat)
    out = torch.empty(1, dtype=torch.float32, device=flat.device)
    nb = _L().pa2d_sumsq_workspace(flat.numel())
    ws = _ws(nb, flat)
    _lib.check(_L().pa2d_sumsq(_p(flat), flat.numel(), _p(out), ws.data_ptr(), nb, _stream()), "sumsq")
    return out


def adamw_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step_index, gnorm_sq=None, max_norm=0.0):
    _chk(p, g, m, v, gnorm_sq)
    _lib.check(_L().pa2d_adamw_step(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, weight_decay,
                                    step_index, _p(gnorm_sq), max_norm, _stream()), "adamw_step")


ADAMW_ROW = 8      # floats of one coefficient row (include/pa2d.h: pa2d_adamw_coefficients)


def adamw_coefficients(lr, beta1, beta2, eps, weight_decay, step_index, max_norm=0.0, out=None):
    """The row `adamw_step_dev` reads: (lr / bias1, 1 - lr wd, 1 - beta1, beta2, 1 - beta2, sqrt(bias2), eps, max_norm),
    evaluated in double and rounded once by the library (the values `adamw_step` hands its kernel).  Host arithmetic
    only.  `out`: a contiguous fp32 HOST tensor of 8 elements to fill (e.g. a pinned staging slot); else a new one."""
    if out is None:
        out = torch.empty(ADAMW_ROW, dtype=torch.float32)
    if out.is_cuda or out.dtype != torch.float32 or out.numel() != ADAMW_ROW or not out.is_contiguous():
        raise ValueError("adamw_coefficients fills a contiguous fp32 host tensor of 8 elements")
    _lib.check(_L().pa2d_adamw_coefficients(float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
                                            int(step_index), float(max_norm), out.data_ptr()), "adamw_coefficients")
    return out


def adamw_step_dev(p, g, m, v, coef, gnorm_sq=None):
    """`adamw_step` with the step's coefficient row `coef` (fp32 [8], on the device, 16-byte aligned) read by the kernel:
    no argument depends on the step, so the launch can be captured."""
    _chk(p, g, m, v, coef, gnorm_sq)
    if coef.numel() != ADAMW_ROW:
        raise ValueError("adamw_step_dev needs a coefficient row of 8 floats")
    _lib.check(_L().pa2d_adamw_step_dev(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(coef), _p(gnorm_sq), _stream()),
               "adamw_step_dev")


def rel_l2_fwd(pred2d, y2d):
    _chk(pred2d, y2d)
    B, L = pred2d.shape
    dn = torch.empty(B, dtype=torch.float32, device=pred2d.device)
    yn, ratio = torch.empty_like(dn), torch.empty_like(dn)
    _lib.check(_L().pa2d_rel_l2_fwd(_p(pred2d), _p(y2d), _p(dn), _p(yn), _p(ratio), B, L, _stream()), "rel_l2_fwd")
    return dn, yn, ratio


def rel_l2_bwd(pred2d, y2d, dn, yn, gout):
    """gout: per-sample upstream gradient [B]."""
    _chk(pred2d, y2d, dn, yn, gout)
    B, L = pred2d.shape
    if gout.numel() != B:
        raise ValueError("gout must hold one value per sample")
    dpred = torch.empty_like(pred2d)
    _lib.check(_L().pa2d_rel_l2_bwd(_p(pred2d), _p(y2d), _p(dn), _p(yn), _p(gout), _p(dpred), B, L, _stream()),
               "rel_l2_bwd")
    return dpred


def _darcy_loss_shapes(out_n, y_n, mean, std, s):
    _chk(out_n, y_n, mean, std)
    if out_n.dim() != 2 or out_n.shape != y_n.shape or out_n.shape[1] != s * s:
        raise ValueError(f"darcy_loss needs out_n, y_n of one shape [B, s*s]; got {tuple(out_n.shape)}, {tuple(y_n.shape)}, s={s}")
    if mean.numel() != 1 or std.numel() != 1:
        raise ValueError("darcy_loss needs a scalar normaliser (mean and std of one element each)")
    return out_n.shape[0]


def darcy_loss_fwd(out_n, y_n, mean, std, dx, s):
    """out_n, y_n [B, s*s]; mean / std: the y-normaliser's one-element tensors, read on the device.
    Returns (sums [3] = (loss, sum l2, sum (dxr + dyr)), norms [6, B])."""
    B = _darcy_loss_shapes(out_n, y_n, mean, std, s)
    sums = torch.empty(3, dtype=torch.float32, device=out_n.device)
    norms = torch.empty(6, B, dtype=torch.float32, device=out_n.device)
    nb = _L().pa2d_darcy_loss_workspace(B, s)
    ws = _ws(nb, out_n)
    _lib.check(_L().pa2d_darcy_loss_fwd(_p(out_n), _p(y_n), _p(mean), _p(std), _p(norms), _p(sums), ws.data_ptr(), nb, B, s,
                                        float(dx), _stream()), "darcy_loss_fwd")
    return sums, norms


def darcy_loss_bwd(out_n, y_n, mean, std, norms, coef, dx, s):
    """coef [2] on the device: the upstream gradients of (sum l2, sum (dxr + dyr)).  Returns d out_n."""
    B = _darcy_loss_shapes(out_n, y_n, mean, std, s)
    _chk(norms, coef)
    if norms.numel() != 6 * B or coef.numel() != 2:
        raise ValueError("darcy_loss_bwd needs norms [6, B] and coef [2]")
    dout = torch.empty_like(out_n)
    _lib.check(_L().pa2d_darcy_loss_bwd(_p(out_n), _p(y_n), _p(mean), _p(std), _p(norms), _p(coef), _p(dout), B, s,
                                        float(dx), _stream()), "darcy_loss_bwd")
    return dout


def _strided_target(pred2d, y, mean, std):
    """(B, L, element stride, batch stride) of the target `y` of a [B, L] prediction.  `y` may be any fp32 GPU view whose
    element (b, i) lies at b * batch_stride + i * elem_stride of its storage: a contiguous [B, L], or a slice such as
    yy[..., t:t+1] of [B, N, 4, T] (no reshape copy)."""
    _chk(pred2d, mean, std)
    if pred2d.dim() != 2 or not y.is_cuda or y.dtype != torch.float32 or y.shape[0] != pred2d.shape[0]:
        raise ValueError("rel_l2_affine needs pred [B, L] and an fp32 GPU target of B samples")
    if (mean is None) != (std is None) or (mean is not None and (mean.numel() != 1 or std.numel() != 1)):
        raise ValueError("rel_l2_affine needs a scalar normaliser (mean and std of one element each) or none")
    B, L = pred2d.shape
    strides = uniform_strides(y)
    if strides is None or y.numel() != B * L:
        raise ValueError("the target is no uniformly strided view of L elements per sample")
    return B, L, strides[0], strides[1]


def uniform_strides(y):
    """(element stride, batch stride) if sample b's elements, in row-major order of y.shape[1:], lie at
    b * batch_stride + i * elem_stride with elem_stride >= 1; else None."""
    es = None
    expect = 1
    for size, stride in zip(reversed(y.shape[1:]), reversed(y.stride()[1:])):
        if size == 1:
            continue
        if es is None:
            es = stride
        if stride != es * expect or es < 1:
            return None
        expect *= size
    return (1 if es is None else es), y.stride(0)


def rel_l2_affine_fwd(pred2d, y, mean=None, std=None):
    """Per-sample ||o - y|| / ||y|| of the decoded prediction o = pred std + mean and target y std + mean (mean / std:
    one-element device tensors, None = identity).  Returns (dnorm, ynorm, ratio), each [B]."""
    B, L, es, bs = _strided_target(pred2d, y, mean, std)
    dn = torch.empty(B, dtype=torch.float32, device=pred2d.device)
    yn, ratio = torch.empty_like(dn), torch.empty_like(dn)
    nb = 4 * 2 * B * _lib.REL_L2_AFFINE_SPLIT
    ws = _ws(nb, pred2d)
    _lib.check(_L().pa2d_rel_l2_affine_fwd(_p(pred2d), _p(y), es, bs, _p(mean), _p(std), _p(dn), _p(yn), _p(ratio),
                                           ws.data_ptr(), nb, B, L, _stream()), "rel_l2_affine_fwd")
    return dn, yn, ratio


def rel_l2_affine_bwd(pred2d, y, mean, std, dn, yn, gout):
    """gout: per-sample upstream gradient [B].  Returns d pred [B, L]."""
    B, L, es, bs = _strided_target(pred2d, y, mean, std)
    _chk(dn, yn, gout)
    if gout.numel() != B or dn.numel() != B or yn.numel() != B:
        raise ValueError("dn, yn and gout must hold one value per sample")
    dpred = torch.empty_like(pred2d)
    _lib.check(_L().pa2d_rel_l2_affine_bwd(_p(pred2d), _p(y), es, bs, _p(mean), _p(std), _p(dn), _p(yn), _p(gout),
                                           _p(dpred), B, L, _stream()), "rel_l2_affine_bwd")
    return dpred


def embed_bias_supported(h, placeholder, tvec):
    """True where pa2d_embed_bias_* apply: fp32 GPU tensors, C % 4 == 0 and 16-byte aligned storage (the kernels move 16
    bytes at a time)."""
    ts = [t for t in (h, placeholder, tvec) if t is not None]
    return (h.dim() == 3 and h.shape[-1] % 4 == 0
            and all(t.is_cuda and t.dtype == torch.float32 and t.data_ptr() % 16 == 0 for t in ts))


def embed_bias_fwd(h, placeholder=None, tvec=None, out=None):
    """z[b, n, :] = (h[b, n, :] + placeholder[:]) + tvec[b, :]; h [B, N, C], placeholder [C], tvec [B, C] (either may be
    None).  `out` may be h itself (in place)."""
    _chk(h, placeholder, tvec, out)
    B, N, C = h.shape
    if (placeholder is not None and placeholder.numel() != C) or (tvec is not None and tuple(tvec.shape) != (B, C)):
        raise ValueError("embed_bias needs placeholder [C] and tvec [B, C]")
    z = torch.empty_like(h) if out is None else out
    _lib.check(_L().pa2d_embed_bias_fwd(_p(h), _p(placeholder), _p(tvec), _p(z), B, N, C, _stream()), "embed_bias_fwd")
    return z


def embed_bias_bwd(dz, want_placeholder, want_tvec):
    """dz [B, N, C] -> (dplaceholder [C] or None, dtvec [B, C] or None): the column sums, by a fixed-order reduction."""
    _chk(dz)
    B, N, C = dz.shape
    dp = torch.empty(C, dtype=torch.float32, device=dz.device) if want_placeholder else None
    dt = torch.empty(B, C, dtype=torch.float32, device=dz.device) if want_tvec else None
    nb = 4 * _lib.EMBED_BIAS_CHUNKS * (B if want_tvec else 1) * C
    ws = _ws(nb, dz)
    _lib.check(_L().pa2d_embed_bias_bwd(_p(dz), _p(dp), _p(dt), ws.data_ptr(), nb, B, N, C, _stream()), "embed_bias_bwd")
    return dp, dt


PREV_SLICE_MAX_M = 64       # widest slice row of pa2d_prev_slice_entry_* (include/pa2d.h)
PREV_SLICE_FWD_ROWS = 64    # rows of one forward chunk (the backward's chunks are longer), and
PREV_SLICE_MAX_UNITS = 4 * 65535      # the (sample, chunk) units of one launch: four per workgroup on a 65535-long grid axis
_EXTENT = 1 << 32           # bytes the kernels' buffer addressing covers


def _prev_slice_entry_shapes(sw, wsw, tb, act):
    """(B, N, M, H) of sw [B, N, M], wsw [H, M], tb [B, H]; raises on what pa2d_prev_slice_entry_* refuse."""
    _chk(sw, wsw, tb)
    if act not in ACT_IDS:
        raise ValueError(f"unknown activation {act!r}")
    if sw.dim() != 3 or wsw.dim() != 2 or tb.dim() != 2:
        raise ValueError(f"prev_slice_entry needs sw [B, N, M], wsw [H, M], tb [B, H]; got {tuple(sw.shape)}, "
                         f"{tuple(wsw.shape)}, {tuple(tb.shape)}")
    (B, N, M), H = sw.shape, wsw.shape[0]
    if wsw.shape[1] != M or tuple(tb.shape) != (B, H):
        raise ValueError(f"prev_slice_entry needs sw [B, N, M], wsw [H, M], tb [B, H]; got {tuple(sw.shape)}, "
                         f"{tuple(wsw.shape)}, {tuple(tb.shape)}")
    if not 1 <= M <= PREV_SLICE_MAX_M:
        raise ValueError(f"prev_slice_entry handles 1 <= M <= {PREV_SLICE_MAX_M} slice weights per point; got {M}")
    if H % 4:
        raise ValueError(f"prev_slice_entry needs a hidden width that is a multiple of 4; got {H}")
    if 4 * max(B * N * H, B * N * M, B * H, H * M) >= _EXTENT:
        raise ValueError("prev_slice_entry: a tensor of 4 GiB or more is outside the kernels' buffer addressing")
    if B * -(-N // PREV_SLICE_FWD_ROWS) > PREV_SLICE_MAX_UNITS:
        raise ValueError(f"prev_slice_entry: B * ceil(N / {PREV_SLICE_FWD_ROWS}) = {B * -(-N // PREV_SLICE_FWD_ROWS)} row chunks "
                         f"are more than the {PREV_SLICE_MAX_UNITS} one launch's grid holds")
    return B, N, M, H


def prev_slice_entry_fwd(sw, wsw, tb, act):
    """h0[b, n, :] = act(sum_m sw[b, n, m] wsw[:, m] + tb[b, :]) in one launch: sw [B, N, M], wsw [H, M], tb [B, H]."""
    B, N, M, H = _prev_slice_entry_shapes(sw, wsw, tb, act)
    h0 = torch.empty(B, N, H, dtype=torch.float32, device=sw.device)
    _lib.check(_L().pa2d_prev_slice_entry_fwd(_p(sw), _p(wsw), _p(tb), _p(h0), B, N, M, H, ACT_IDS[act], _stream()),
               "prev_slice_entry_fwd")
    return h0


def prev_slice_entry_bwd(dh0, sw, wsw, tb, act):
    """dh0 [B, N, H] -> (dwsw [H, M], dtb [B, H]) with the pre-activation recomputed; fixed-order reductions."""
    B, N, M, H = _prev_slice_entry_shapes(sw, wsw, tb, act)
    _chk(dh0)
    if tuple(dh0.shape) != (B, N, H):
        raise ValueError(f"prev_slice_entry_bwd needs dh0 {(B, N, H)}; got {tuple(dh0.shape)}")
    dwsw = torch.empty(H, M, dtype=torch.float32, device=sw.device)
    dtb = torch.empty(B, H, dtype=torch.float32, device=sw.device)
    nb = _L().pa2d_prev_slice_entry_workspace(B, N, M, H)
    ws = _ws(nb, sw)
    _lib.check(_L().pa2d_prev_slice_entry_bwd(_p(dh0), _p(sw), _p(wsw), _p(tb), _p(dwsw), _p(dtb), ws.data_ptr(), nb, B, N,
                                              M, H, ACT_IDS[act], _stream()), "prev_slice_entry_bwd")
    return dwsw, dtb


# ---------------------------------------------------------------------------------------------- velocity-field step tail
WINDOW_SPLIT, WINDOW_MAX_K, WINDOW_MAX_F = _lib.WINDOW_SPLIT, _lib.WINDOW_MAX_K, _lib.WINDOW_MAX_F


def _column_window(pred, yy, col0, what):
    """(B, N, k, pointer of yy[0, 0, col0], row stride, batch stride) for pred [B, N, k] and the columns [col0, col0 + k) of
    yy [B, N, W]: any fp32 GPU view with unit stride along its last axis (yy[..., :T] of a longer tensor included)."""
    _chk(pred)
    if pred.dim() != 3 or yy.dim() != 3 or tuple(yy.shape[:2]) != tuple(pred.shape[:2]):
        raise ValueError(f"{what} needs pred [B, N, k] and a target [B, N, W]; got {tuple(pred.shape)}, {tuple(yy.shape)}")
    if not yy.is_cuda or yy.dtype != torch.float32 or (yy.shape[-1] > 1 and yy.stride(-1) != 1):
        raise ValueError(f"{what} needs an fp32 GPU target with unit stride along its last axis")
    B, N, k = pred.shape
    if not 0 <= col0 <= yy.shape[-1] - k:
        raise ValueError(f"{what}: columns [{col0}, {col0 + k}) are outside a target of {yy.shape[-1]} columns")
    if not 1 <= k <= WINDOW_MAX_K:
        raise ValueError(f"{what} handles 1 <= k <= {WINDOW_MAX_K} columns per prediction; got {k}")
    return B, N, k, _p(yy, col0), yy.stride(1), yy.stride(0)


def rel_l2_window_fwd(pred, yy, col0):
    """Per-sample ||pred - yy[..., col0:col0+k]|| / ||yy[..., col0:col0+k]|| with the target read where it lies.
    Returns (dnorm, ynorm, ratio), each [B]."""
    B, N, k, yp, rs, bs = _column_window(pred, yy, col0, "rel_l2_window")
    dn = torch.empty(B, dtype=torch.float32, device=pred.device)
    yn, ratio = torch.empty_like(dn), torch.empty_like(dn)
    nb = 4 * 2 * B * WINDOW_SPLIT
    ws = _ws(nb, pred)
    _lib.check(_L().pa2d_rel_l2_window_fwd(_p(pred), yp, rs, bs, _p(dn), _p(yn), _p(ratio), ws.data_ptr(), nb, B, N, k,
                                           _stream()), "rel_l2_window_fwd")
    return dn, yn, ratio


def rel_l2_window_bwd(pred, yy, col0, dn, yn, gout):
    """gout: per-sample upstream gradient [B].  Returns d pred [B, N, k]."""
    B, N, k, yp, rs, bs = _column_window(pred, yy, col0, "rel_l2_window")
    _chk(dn, yn, gout)
    if gout.numel() != B or dn.numel() != B or yn.numel() != B:
        raise ValueError("dn, yn and gout must hold one value per sample")
    dpred = torch.empty_like(pred)
    _lib.check(_L().pa2d_rel_l2_window_bwd(_p(pred), yp, rs, bs, _p(dn), _p(yn), _p(gout), _p(dpred), B, N, k, _stream()),
               "rel_l2_window_bwd")
    return dpred


def rollout_record(nsteps, B, like):
    """The record [S, B, WINDOW_SPLIT, 2] that `rollout_tail` fills step by step and `rollout_score` reduces."""
    return torch.empty(nsteps, B, WINDOW_SPLIT, 2, dtype=torch.float32, device=like.device)


def rollout_tail(pred, window, traj=None, col=0, yy=None, ycol=0, record=None, s=0):
    """One launch after a model call of a no-grad rollout: `window` [B, N, F] is shifted by k columns in place and `pred`
    [B, N, k] appended; traj [B, N, T] (optional) receives pred in columns [col, col + k); with a target yy [B, N, W]
    (optional; columns [ycol, ycol + k) are this step's) the step's partial sums go into slot `s` of `record`."""
    _chk(pred, window, traj, record)
    if window.dim() != 3 or pred.dim() != 3 or tuple(window.shape[:2]) != tuple(pred.shape[:2]):
        raise ValueError(f"rollout_tail needs pred [B, N, k] and a window [B, N, F]; got {tuple(pred.shape)}, "
                         f"{tuple(window.shape)}")
    (B, N, k), F = pred.shape, window.shape[-1]
    if not 1 <= k <= min(F, WINDOW_MAX_K) or F > WINDOW_MAX_F:
        raise ValueError(f"rollout_tail handles 1 <= k <= min(F, {WINDOW_MAX_K}) and F <= {WINDOW_MAX_F}; got k = {k}, F = {F}")
    T = 0
    if traj is not None:
        if traj.dim() != 3 or tuple(traj.shape[:2]) != (B, N) or not 0 <= col <= traj.shape[-1] - k:
            raise ValueError(f"rollout_tail: columns [{col}, {col + k}) do not lie in a trajectory buffer {tuple(traj.shape)}")
        T = traj.shape[-1]
    yp = rs = bs = S = 0
    if yy is not None:
        _, _, _, yp, rs, bs = _column_window(pred, yy, ycol, "rollout_tail")
        if record is None or record.dim() != 4 or tuple(record.shape[1:]) != (B, WINDOW_SPLIT, 2) or not 0 <= s < record.shape[0]:
            raise ValueError("rollout_tail: a target needs a record [S, B, WINDOW_SPLIT, 2] and a step index inside it")
        S = record.shape[0]
    _lib.check(_L().pa2d_rollout_tail(_p(pred), _p(window), _p(traj), T, col, yp, rs, bs, _p(record), s, S, B, N, k, F,
                                      _stream()), "rollout_tail")


def rollout_score(record, N):
    """(step_ratio [S, B], full_ratio [B]) of a record that S `rollout_tail` calls on [B, N, .] tensors filled."""
    _chk(record)
    S, B = record.shape[:2]
    step_ratio = torch.empty(S, B, dtype=torch.float32, device=record.device)
    full_ratio = torch.empty(B, dtype=torch.float32, device=record.device)
    _lib.check(_L().pa2d_rollout_score(_p(record), _p(step_ratio), _p(full_ratio), S, B, N, _stream()), "rollout_score")
    return step_ratio, full_ratio
