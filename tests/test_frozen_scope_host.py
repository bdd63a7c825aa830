"""Host-side contract of `ops.weights_frozen()` (one table per scope: `_scoped`, `refresh`, re-entry, `unscoped`, the three
read-only views) and of the call sequences `functional.attn_forward` / `attn_backward` / `EncodeFn` issue to `ops`, recorded
through stand-ins in the style of test_block_tail_host._record.  CPU tensors and fake makers: nothing native runs."""
import pytest
import torch

from transformerbasednavierstokesolver_amd import _lib, ops
from transformerbasednavierstokesolver_amd import functional as Fn


# ---------------------------------------------------------------------------------------------- the scope table
def _maker(log):
    def make(buf):
        log.append(buf.data_ptr())
    return make


def test_scoped_makes_once_per_key_and_refresh_remakes_in_place():
    w, v = torch.zeros(4), torch.zeros(4)
    made_w, made_v = [], []
    assert ops._scoped(("image", 1), 32, _maker(made_w), (w,)) == 0 and not made_w       # outside any scope
    with ops.weights_frozen() as scope:
        p = ops._scoped(("image", 1), 32, _maker(made_w), (w,))
        assert p != 0 and made_w == [p]
        assert ops._scoped(("image", 1), 32, _maker(made_w), (w,)) == p and made_w == [p]      # a hit: same pointer, no make
        q = ops._scoped(("image", 2), 48, _maker(made_v), (v,))
        assert q not in (0, p) and made_v == [q]
        assert {k: (keep, buf.numel()) for k, (keep, buf, _) in scope.table.items()} == {("image", 1): ((w,), 32),
                                                                                        ("image", 2): ((v,), 48)}
        scope.refresh()
        assert made_w == [p, p] and made_v == [q, q]          # every entry once, into the same buffer
    assert not ops._frozen
    scope.refresh()                                           # a scope outlives its `with` (GraphedRollout keeps one)
    assert made_w == [p, p, p] and made_v == [q, q, q]


def test_nested_scopes_are_independent_and_reentry_sees_earlier_entries():
    w, made = torch.zeros(4), []
    with ops.weights_frozen() as outer:
        a = ops._scoped(("image", 1), 16, _maker(made), (w,))
        with ops.weights_frozen() as inner:
            b = ops._scoped(("image", 1), 16, _maker(made), (w,))
            assert b not in (0, a) and list(inner.table) == [("image", 1)]
        assert ops._scoped(("image", 1), 16, _maker(made), (w,)) == a and len(outer.table) == 1
    assert made == [a, b] and not ops._frozen
    with ops.weights_frozen(outer) as again:
        assert again is outer
        assert ops._scoped(("image", 1), 16, _maker(made), (w,)) == a        # the earlier entry: no make
        c = ops._scoped(("image", 3), 16, _maker(made), (w,))
    assert made == [a, b, c] and len(outer.table) == 2 and not ops._frozen
    with pytest.raises(ZeroDivisionError):
        with ops.weights_frozen(outer):
            1 / 0
    assert not ops._frozen


def test_unscoped_adds_nothing_and_returns_zero():
    w, made = torch.zeros(4), []
    with ops.weights_frozen() as scope:
        with ops.unscoped():
            assert ops._scoped(("image", 1), 16, _maker(made), (w,)) == 0
            with ops.weights_frozen() as inner:           # a scope opened under it works as usual
                assert ops._scoped(("image", 1), 16, _maker(made), (w,)) != 0 and len(inner.table) == 1
            assert ops._scoped(("image", 2), 16, _maker(made), (w,)) == 0
        assert not scope.table and len(made) == 1
        assert ops._scoped(("image", 1), 16, _maker(made), (w,)) != 0
    assert not ops._frozen
    with ops.unscoped():                                  # outside any scope: nothing to suspend
        assert ops._scoped(("image", 1), 16, _maker(made), (w,)) == 0
    assert not ops._frozen


class _FakeLib:
    """Every bound symbol of the C ABI as a recorder: the argument count is checked against `_lib.SIGNATURES`, size
    queries return 64 bytes, `*_supported` 1, everything else 0 (success)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name not in _lib.SIGNATURES:
            raise AttributeError(name)

        def fn(*args):
            assert len(args) == len(_lib.SIGNATURES[name][1]), (name, len(args))
            self.calls.append(name)
            return 64 if name.endswith("_bytes") or "workspace" in name else int(name.endswith("_supported"))
        return fn


@pytest.fixture
def fake_lib(monkeypatch):
    lib = _FakeLib()
    monkeypatch.setattr(ops, "_L", lambda: lib)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "_chk", lambda *ts: None)
    monkeypatch.setattr(ops, "_chk_act", lambda *ts: any(t is not None and t.dtype == torch.bfloat16 for t in ts))
    return lib


def test_views_expose_the_key_layouts_of_the_callers(fake_lib):
    """The conv wrappers, the linears and the fused tail inside one scope, on CPU tensors over the recording library: the
    three views hold (w ptrs, dims, direction, engine) -> (weights..., buffer) as their readers expect."""
    B, H, W, D, C = 2, 3, 4, 2, 8
    z = torch.zeros
    wx, wf, w1, b = z(C, C, 3, 3), z(C, C, 3, 3), z(C, C, 3, 3), z(C)
    wx3, wf3 = z(C, C, 3, 3, 3), z(C, C, 3, 3, 3)
    x, x3, wl = z(B, H * W, C), z(B, H * W * D, C), z(2 * C, C)
    S, S16 = ops.ENGINE_SPLIT, ops.ENGINE_BF16S
    with ops.weights_frozen() as scope:
        ops.conv3x3x2_fwd(x, wx, b, wf, b, H, W, engine="split")
        ops.conv3x3x2_bwd(z(B, H * W, 2 * C), x, wx, wf, H, W, engine="split")
        ops.conv3x3x2_bwd(z(B, H * W, 2 * C), x, wx, wf, H, W, need_dx=False, engine="split")     # no pack without dx
        ops.conv3x3x2_fwd(x.bfloat16(), wx, b, wf, b, H, W)
        ops.conv3x3x2_fwd_planes(z(64, dtype=torch.uint8), wx, b, wf, b, B, H, W, "split")       # shares the 3x3 pack
        ops.conv3x3x2_bwd_planes(z(64, dtype=torch.uint8), z(64, dtype=torch.uint8), wx, wf, B, H, W, "split")
        ops.conv3x3x3x2_fwd(x3, wx3, b, wf3, b, H, W, D, engine="split")
        ops.conv3x3x3x2_bwd(z(B, H * W * D, 2 * C), x3, wx3, wf3, H, W, D, engine="split")
        ops.conv3x3_fwd(x, w1, b, H, W, engine="split")
        ops.conv3x3_bwd(x, x, w1, H, W, engine="split")
        ops.linear_fwd(x.view(-1, C), wl, engine="split")
        ops.linear_bwd_data(z(B * H * W, 2 * C), wl, engine="split")
        ops.block_tail_fwd(z(B, H * W, 2 * C), 2 * C, 0, z(B * 2, 4, C // 2), z(4, C // 2), z(4), z(2), z(B * H * W, C), z(C, C),
                           b, b, b, wl, z(2 * C), wl.t().contiguous(), b, None, None, B, H * W, 2, C // 2, 4, "gelu",
                           engine="split")
        n_calls = len(fake_lib.calls)
        pk = lambda a, c, depth, d, e: (a.data_ptr(), c.data_ptr(), B, H, W, depth, C, d, e)
        assert set(scope.packs) == {pk(wx, wf, None, 0, S), pk(wx, wf, None, 1, S), pk(wx, wf, None, 0, S16),
                                    pk(wx3, wf3, D, 0, S), pk(wx3, wf3, D, 1, S)}
        keep = scope.packs[pk(wx3, wf3, D, 1, S)]
        assert keep[0] is wx3 and keep[1] is wf3 and keep[2].dtype == torch.uint8 and keep[2].numel() == 64
        assert set(scope.packs1) == {(w1.data_ptr(), B, H, W, C, 0, S), (w1.data_ptr(), B, H, W, C, 1, S)}
        assert scope.packs1[(w1.data_ptr(), B, H, W, C, 0, S)][0] is w1
        tails = [k for k in scope.images if k[1] == "tail"]
        assert set(scope.images) - set(tails) == {(wl.data_ptr(), 0, 2 * C, C, S), (wl.data_ptr(), 1, C, 2 * C, S)}
        assert len(tails) == 3 and (wl.data_ptr(), "tail", 2 * C, C, S) in tails
        assert scope.images[(wl.data_ptr(), 0, 2 * C, C, S)][0] is wl
        assert len(scope.table) == len(scope.packs) + len(scope.packs1) + len(scope.images) == 12
        for view in (scope.packs, scope.packs1, scope.images):
            with pytest.raises(TypeError):
                view[(0,)] = None
        scope.refresh()
        remade = fake_lib.calls[n_calls:]
        assert len(remade) == 12 and all("pack" in n or "image" in n for n in remade)
    assert not ops._frozen


def test_engine_refusals_keep_their_words(fake_lib):
    x, w, b = torch.zeros(1, 4, 8), torch.zeros(8, 8, 3, 3), torch.zeros(8)
    with pytest.raises(ValueError, match="the single 3x3 conv has no bf16-storage variant; use the f32, split or bf16 engine"):
        ops.conv3x3_fwd(x, w, b, 2, 2, engine="bf16s")
    with pytest.raises(ValueError, match="the single 3x3 conv has no bf16-storage variant"):
        ops.conv3x3_bwd(x, x, w, 2, 2, engine="bf16s")
    w3 = torch.zeros(8, 8, 3, 3, 3)
    for bad in (dict(engine="bf16s"), dict(engine="split", x=x.bfloat16())):
        xx = bad.pop("x", x)
        with pytest.raises(NotImplementedError, match=r"bf16 storage \(engine 'bf16s'\) is not implemented for the 3-D structured mesh"):
            ops.conv3x3x3x2_fwd(xx, w3, b, w3, b, 2, 2, 1, **bad)
        with pytest.raises(NotImplementedError, match="not implemented for the 3-D structured mesh"):
            ops.conv3x3x3x2_bwd(torch.zeros(1, 4, 16, dtype=xx.dtype), xx, w3, w3, 2, 2, 1, **bad)
    with pytest.raises(ValueError, match=r"need xn \[B, H\*W, C\] and w \[C, C, 3, 3\]"):
        ops.conv3x3_fwd(x, w, b, 2, 3, engine="split")
    with pytest.raises(ValueError, match=r"conv3x3x3x2_fwd: N = 4 is not H\*W\*depth = 2\*2\*2"):
        ops.conv3x3x3x2_fwd(x, w3, b, w3, b, 2, 2, 2, engine="split")
    assert not fake_lib.calls


# ---------------------------------------------------------------------------------------------- call sequences
B, HEADS, D, M = 2, 2, 4, 3
C = HEADS * D
GEOM = {"2d": (3, 4), "3d": (2, (3, 2)), "planes": (3, 4), "irregular": (None, None)}       # N = 12 points each
N = 12
PROJ_FWD = {"2d": "conv3x3x2_fwd", "3d": "conv3x3x3x2_fwd", "planes": "conv3x3x2_fwd_planes", "irregular": "linear_fwd"}
DROP = ((429496729, 1.25, 7, 0), (429496729, 1.25, 7, 64))


def _record(monkeypatch):
    """Stand-ins for every `ops` function the attention forward and backward reach: they record (name, first weight
    argument where the scope matters) and return zeros of the right shape."""
    calls, weights = [], []
    z = torch.zeros

    def conv_fwd(xn, wx, *a, **k):
        return z(xn.shape[0], xn.shape[1], 2 * wx.shape[0])

    def conv_fwd_planes(xn_planes, wx, bx, wf, bf, B_, H, W, engine):
        return z(B_, H * W, 2 * wx.shape[0])

    def image(w):
        """What the real linears do with their weight inside a scope."""
        weights.append(w)
        ops._scoped(("image", w.data_ptr()), 16, lambda buf: None, (w,))

    def linear_fwd(x2d, w, bias=None, res=None, act=None, want_pre=False, engine=None, save_derivative=False):
        image(w)
        return z(x2d.shape[0], w.shape[0]), None

    def linear_bwd_data(dy, w, pre=None, act=None, engine=None, pre_is_derivative=False):
        image(w)
        return z(dy.shape[0], w.shape[1])

    def linear_bwd_weight(dy, x2d, want_bias=True, engine=None, into=None):
        return z(dy.shape[1], x2d.shape[1]), z(dy.shape[1])

    def slice_scatter(xm, ldx, xo, v, ldv, vo, ws_w, bs, temperature, B_, N_, heads, D_, M_, want_norm=True, **k):
        return z(B_ * heads, 1, M_, D_), (z(B_ * heads, 1, M_) if want_norm else None)

    def token_attn_fwd(spart, npart, wq, wk, wv, drop=None):
        BH, _, M_, D_ = spart.shape
        return z(BH, M_, D_), z(BH, M_), z(BH, M_, D_)

    def token_attn_bwd(s, nrm, wq, wk, wv, dopart, into=None, drop=None):
        return torch.zeros_like(s), torch.zeros_like(nrm), z(D, D), z(D, D), z(D, D)

    def deslice_fwd(xm, ldx, xo, o, ws_w, bs, temperature, B_, N_, heads, D_, M_, **k):
        return z(B_, N_, heads * D_)

    def dropout_residual(zz, res, drop):
        return torch.zeros_like(zz)

    def slice_bwd_points(xf, dy, ws_w, bs, temperature, o, ds, dn, B_, N_, heads, D_, M_, **k):
        return torch.zeros_like(xf), torch.zeros_like(ws_w), torch.zeros_like(bs), z(heads)

    def slice_bwd_points_planes(xf, dy, ws_w, bs, temperature, o, ds, dn, nrm, B_, N_, heads, D_, M_, engine, **k):
        return z(64, dtype=torch.uint8), z(C), z(C), torch.zeros_like(ws_w), torch.zeros_like(bs), z(heads)

    def conv_bwd(dout, xn, wx, wf, *a, need_dx=True, **k):
        return (torch.zeros_like(xn) if need_dx else None), torch.zeros_like(wx), z(C), torch.zeros_like(wf), z(C)

    def conv_bwd_planes(doutp, xnp, wx, wf, B_, H, W, engine, need_dx=True, into=None):
        return (z(B_, H * W, C) if need_dx else None), torch.zeros_like(wx), torch.zeros_like(wf)

    fakes = dict(conv3x3x2_fwd=conv_fwd, conv3x3x3x2_fwd=conv_fwd, conv3x3x2_fwd_planes=conv_fwd_planes, linear_fwd=linear_fwd,
                 linear_bwd_data=linear_bwd_data, linear_bwd_weight=linear_bwd_weight, slice_scatter=slice_scatter,
                 token_attn_fwd=token_attn_fwd, token_attn_bwd=token_attn_bwd, deslice_fwd=deslice_fwd,
                 dropout_residual=dropout_residual, slice_bwd_points=slice_bwd_points,
                 slice_bwd_points_planes=slice_bwd_points_planes, conv3x3x2_bwd=conv_bwd, conv3x3x3x2_bwd=conv_bwd,
                 conv3x3x2_bwd_planes=conv_bwd_planes)
    for name, fn in fakes.items():
        def spy(*a, _f=fn, _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, spy)
    return calls, weights


def _params(case, keys=Fn.ATTN_KEYS):
    g = torch.Generator().manual_seed(0)
    wshape = {"2d": (C, C, 3, 3), "3d": (C, C, 3, 3, 3), "planes": (C, C, 3, 3), "irregular": (C, C)}[case]
    shapes = dict(temperature=(1, HEADS, 1, 1), wx=wshape, bx=(C,), wf=wshape, bf=(C,), ws=(M, D), bs=(M,), wq=(D, D),
                  wk=(D, D), wv=(D, D), wo=(C, C), bo=(C,))
    return {k: torch.randn(*shapes[k], generator=g) for k in keys}


def _attn_forward(case, P, drop):
    H, W = GEOM[case]
    res = torch.zeros(B, N, C)
    if case == "planes":
        return Fn.attn_forward(None, P, res, H, W, HEADS, "split", xn_planes=torch.zeros(64, dtype=torch.uint8), shape=(B, N, C),
                               drop=drop)
    return Fn.attn_forward(torch.zeros(B, N, C), P, res, H, W, HEADS, "split", drop=drop)


BWD_PREFIX = ["linear_bwd_data", "linear_bwd_weight", "slice_scatter", "token_attn_bwd"]
BWD_SUFFIX = {"2d": ["slice_bwd_points", "conv3x3x2_bwd"], "3d": ["slice_bwd_points", "conv3x3x3x2_bwd"],
              "planes": ["slice_bwd_points_planes", "conv3x3x2_bwd_planes"],
              "irregular": ["slice_bwd_points", "linear_bwd_weight", "linear_bwd_data"]}


@pytest.mark.parametrize("drop", [None, DROP])
@pytest.mark.parametrize("case", list(GEOM))
def test_attention_call_sequences(monkeypatch, case, drop):
    calls, _ = _record(monkeypatch)
    P = _params(case)
    H, W = GEOM[case]
    out, saved = _attn_forward(case, P, drop)
    assert tuple(out.shape) == (B, N, C)
    want = [PROJ_FWD[case], "slice_scatter", "token_attn_fwd", "deslice_fwd", "linear_fwd"]
    assert calls == want + (["dropout_residual"] if drop else []), calls
    for need_dx in (True, False):
        del calls[:]
        dxn, g = Fn.attn_backward(saved, P, torch.zeros(B, N, C), H, W, HEADS, need_dx=need_dx, engine="split",
                                  planes=case == "planes", drop=drop)
        suffix = [n for n in BWD_SUFFIX[case] if need_dx or case != "irregular" or n != "linear_bwd_data"]
        assert calls == (["dropout_residual"] if drop else []) + BWD_PREFIX + suffix, calls
        assert (dxn is not None) == need_dx and (dxn is None or tuple(dxn.shape) == (B, N, C))
        assert set(g) == set(Fn.ATTN_KEYS) and all(g[k].shape == P[k].shape for k in g), {k: g[k].shape for k in g}


@pytest.mark.parametrize("case", ["2d", "3d", "planes"])
def test_attention_backward_with_targets_returns_no_gradients(monkeypatch, case):
    """Structured meshes with gradient buffers: every backward op gets its `into`, one return, no dict."""
    calls, _ = _record(monkeypatch)
    P = _params(case)
    H, W = GEOM[case]
    _, saved = _attn_forward(case, P, None)
    del calls[:]
    targets = {k: torch.zeros_like(v) for k, v in P.items()}
    dxn, g = Fn.attn_backward(saved, P, torch.zeros(B, N, C), H, W, HEADS, engine="split", targets=targets,
                              planes=case == "planes")
    assert g is None and tuple(dxn.shape) == (B, N, C) and calls == BWD_PREFIX + BWD_SUFFIX[case]


def test_encode_call_sequence(monkeypatch):
    calls, _ = _record(monkeypatch)
    P = _params("2d", Fn.ENC_KEYS)
    params = [P[k].requires_grad_() for k in Fn.ENC_KEYS]
    xn = torch.zeros(B, N, C, requires_grad=True)
    code, xm = Fn.attention_encode(xn, 3, 4, HEADS, params, engine="split")
    assert calls == ["conv3x3x2_fwd", "slice_scatter", "token_attn_fwd"], calls
    assert tuple(code.shape) == (B, HEADS, M, D) and tuple(xm.shape) == (B, N, C)
    del calls[:]
    (code.sum() + xm.sum()).backward()
    assert calls == ["token_attn_bwd", "slice_bwd_points", "conv3x3x2_bwd"], calls
    assert xn.grad is not None and all(p.grad is not None and p.grad.shape == p.shape for p in params)


def test_block_tail_front_half(monkeypatch):
    calls, _ = _record(monkeypatch)

    def block_tail_fwd(xm, ldx, xo, o, ws_w, bs, temperature, fx2d, *a, **k):
        calls.append("block_tail_fwd")
        return torch.zeros_like(fx2d), None, None
    monkeypatch.setattr(ops, "block_tail_fwd", block_tail_fwd)
    for case in ("2d", "3d", "irregular"):
        del calls[:]
        H, W = GEOM[case]
        fx = torch.zeros(B, N, C)
        z = torch.zeros
        with torch.no_grad():
            out, nxt = Fn.block_tail(fx, fx, _params(case), H, W, HEADS, z(C), z(C), "gelu", z(C, C), z(C), z(C, C), z(C))
        assert calls == [PROJ_FWD[case], "slice_scatter", "token_attn_fwd", "block_tail_fwd"], calls
        assert tuple(out.shape) == (B, N, C) and nxt is None


# ---------------------------------------------------------------------------------------------- temporaries and the scope
def test_irregular_stacked_weight_is_made_once_and_never_enters_a_scope(monkeypatch):
    """The stacked [wx; wf] of the irregular mesh is a temporary: its linears run under `ops.unscoped()`, so a scope ends up
    holding parameters only, however many calls run inside it; the backward reuses the forward's tensor."""
    calls, weights = _record(monkeypatch)
    P = _params("irregular")
    with ops.weights_frozen() as scope:
        for it in range(2):
            del weights[:]
            _, saved = Fn.attn_forward(torch.zeros(B, N, C), P, None, None, None, HEADS, "split")
            Fn.attn_backward(saved, P, torch.zeros(B, N, C), None, None, HEADS, engine="split")
            assert [tuple(w.shape) for w in weights] == [(2 * C, C), (C, C), (C, C), (2 * C, C)]
            assert weights[0] is weights[3] and weights[1] is P["wo"] and weights[2] is P["wo"]
            assert [keep for keep, _, _ in scope.table.values()] == [(P["wo"],)], it
    assert not ops._frozen


def test_to_out_twice_keeps_its_doubled_weight_out_of_the_scope(monkeypatch):
    calls, weights = _record(monkeypatch)
    w, b = torch.randn(C, C, requires_grad=True), torch.randn(C, requires_grad=True)
    y = torch.zeros(B, N, C, requires_grad=True)
    with ops.weights_frozen() as scope:
        Fn.to_out_twice(y, w, b, engine="split").sum().backward()
        assert calls == ["linear_fwd", "linear_bwd_data", "linear_bwd_weight"] and weights[0] is weights[1]
        assert torch.equal(weights[0], 2.0 * w.detach()) and not scope.table
