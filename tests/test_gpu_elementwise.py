"""Element-wise parity of every stage-kernel family against fp64 (tests/elementwise_check.py), at the shapes where the
dispatch switches kernels.  Every case runs its op through `poisoned` (outputs land in NaN / 1.2e30-filled buffers:
unwritten or run-to-run different elements fail), bounds every element against an fp64 reference computed on the
device (plain fp64 torch for the GEMM-shaped ops, the oracle's formulas for the slice path) and keeps the whole-tensor
rel-L2 assertion of tests/test_gpu_stages.py beside it.

Bounds (TAU / ROW_TOL in elementwise_check.py): |got - ref| <= tau * scale (+ 2^-8 |ref| for bf16-stored outputs), scale =
the same operation on absolute values.  Families: "fwd" (contraction over a layer width: linear forward and data
gradient, conv forward and data gradient, head), "wgrad" (contraction over the rows: weight / bias gradients), "slice"
(scatter, de-slice, slice-backward parameter gradients).  CALIBRATION (MI355X, worst |got - ref| / scale per engine and
family, and the chosen tau; the bounds are at most 4x the worst value seen):

    engine  family  worst     tau      worst case
    f32     fwd     5.2e-7    1.6e-6   linear M=32895 N=1024 K=128 pre-activation
    split   fwd     5.2e-7    1.6e-6   the same case (row-stationary kernel, and with PA2D_LIN_ROWPANEL=off)
    bf16s   fwd     1.3e-3    5e-3     linear M=32968 N=192 K=96 data gradient (saved derivative); + 2^-8 |ref|
    f32     wgrad   2.6e-7    1e-6     linear M=200 N=64 K=64 weight gradient
    split   wgrad   2.6e-7    1e-6     the same case
    bf16s   wgrad   7.9e-8    3e-7     conv 1x12x20 C=64 dwx
    f32     slice   9.1e-6    2e-5     slice B=2 N=4113 heads=8 D=32 M=64 dfx_mid
    split   slice   4.6e-6    1e-5     slice B=1 N=4100 heads=8 D=16 M=128 dfx_mid
    bf16s   slice   5.7e-6    1.2e-5   slice B=1 N=4100 heads=8 D=16 M=128 scatter S
    f32     rows    4.9e-6    1.9e-5   slice B=2 N=4113 heads=8 D=32 M=64 dn (per-row rel-L2)
    split   rows    2.3e-6    9e-6     slice B=1 N=4100 heads=8 D=16 M=128 dn
    bf16s   rows    2.4e-3    9e-3     LayerNorm rows=300 C=64 forward

The corruptions each bound rejects are emulated on the host in test_elementwise_check.py (a one-plane 16 x 16 block:
6.5e-4, four rows x (1 + 1e-4): 3.3e-5, a two-plane 77-row tail: 2.0e-6, two-plane rows 12-15 / 28-31: 2.7e-6, a conv
border ring x (1 + 1e-5): 4.3e-6, a skipped tile: 0.26).  The slice point gradients are checked element-wise against
sum-of-products scales rather than per row: on the exact engine their per-row rel-L2 reaches 2.6e-4 on points whose
softmax weights are nearly one-hot (dL/dlogit cancels), which says nothing about the kernel.  The same run printed the
table at the end of the module (pytest -s).

Kernel coverage (rocprofv3 --kernel-trace over this file lists each of them):

    linear   gemm_rowpanel_kernel          M in {32768, 32769, 32895, 66253}, N in {128, 256, 384, 1024}, K in {128, 256}
             gemm_panel_kernel             N = 192: M = 32968 (256 tiles + 200-row tail) / PA2D_LIN_ROWPANEL=off
             gemm_kc_split_kernel          64x64 small split (M = 24448: 382 tiles, 4096, 256), bf16 storage (128x128 bf16)
             gemm_kc_kernel                exact fp32 (engine f32, M = 24576: 384 tiles, M < 256, K = 12 / 76, switches off)
             gemm_mc_* weight gradient     every linear weight / bias gradient
    conv     conv_halo_kernel              16x16x32 and 32x32x16 (float), bf16 (bf16 storage), auto / force, 421 x 421
             gemm_kc_split_kernel          conv: 256x128 (split_big, M % 256 == 0, >= 512 tiles), 128x128 (508 tiles,
                                           M % 256 != 0), 64x128 (< 256 tiles)
             gemm_kc_kernel (im2col)       engine f32; Cin = 48 (Cin % 32 != 0: 16-wide K-step)
             gemm_mc_planes_kernel / gemm_mc_planes_big_kernel   PA2D_MC_BIG on / off
    slice    scatter3_kernel, deslice3_kernel, slice_bwd3_kernel (split, bf16 storage; M = 128 / D = 16 included)
             exact-fp32 scatter / de-slice / slice-backward kernels (engine f32), token attention forward / backward
    rows     LayerNorm forward / backward (fp32 and bf16 storage), head forward / backward
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from elementwise_check import BF16_STORAGE_REL, ROW_TOL, TAU, check_products, check_rows, poisoned

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_TOL, BWD_TOL = 3e-6, 2e-5          # the whole-tensor rel-L2 bounds of test_gpu_stages.py
BF_TOL = 1e-2                          # ... and of test_gpu_bf16_storage.py
ENV_KEYS = ("PA2D_LIN_ROWPANEL", "PA2D_LIN_PANEL", "PA2D_LIN_SMALL_SPLIT", "PA2D_CONV_HALO", "PA2D_CONV_MFMA", "PA2D_MC_BIG")

WORST = {}      # (engine, family) -> [(|err| / scale, case), ...]: the largest three are printed at the end of the module


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst element-wise error per engine / family (|got - ref| / scale; rows: per-row rel-L2):")
    for k in sorted(WORST):
        for v, case in sorted(WORST[k], reverse=True)[:3]:
            print(f"  {k[0]:6s} {k[1]:6s} {v:.3e}   {case}")


def _note(engine, fam, label, v):
    WORST.setdefault((engine, fam), []).append((v, label))


def _prod(got, ref, scale, engine, fam, label, hw=None):
    bf_out = got.dtype == torch.bfloat16
    v = check_products(got, ref, scale, TAU[(engine, fam)], rel_ref=BF16_STORAGE_REL if bf_out else 0.0, hw=hw,
                       label=f"[{engine}] {label}")
    _note(engine, fam, label, v)


def _rows(got, ref, engine, label, hw=None):
    v = check_rows(got, ref, ROW_TOL[engine], hw=hw, label=f"[{engine}] {label}")
    _note(engine, "rows", label, v)


def _set_env(kernel_env, **kv):
    kernel_env(**{k: kv.get(k) for k in ENV_KEYS})


def _r(rng, *shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32)).to(DEV)


def _store(t, engine):
    """The activation as the engine stores it, and the fp64 copy of exactly those values."""
    t = t.bfloat16() if engine == "bf16s" else t
    return t.contiguous(), t.double()


def _act_and_grad(act, pre):
    """act(pre), act'(pre) in fp64"""
    from oracle import transolver_oracle as orc
    p = pre.detach().clone().requires_grad_(True)
    y = orc._ACTS[act](p)
    y.backward(torch.ones_like(p))
    return y.detach(), p.grad


# ---------------------------------------------------------------------------------------------- linears
# Shapes derived from the dispatch (pa2d_gemm.hip launch_kc): rowpanel_applies (split engine, K in {128, 256}, N % 128 == 0,
# N <= 1024, M / 128 >= 256 rounds; the < 128-row tail goes to the per-tile kernels), panel_applies (split, K % 32 == 0,
# (M / 256) * ceil(N / 128) >= 256; < 256-row tail per tile), kc_split_small_applies (split, K % 32 == 0, K >= 64, N >= 64,
# M >= 256, ceil(M / 128) * ceil(N / 128) < 384), else the exact-fp32 per-tile kernel; bf16 storage: 128x128 bf16 tiles.
LIN_CASES = [  # M, N, K, act, residual, split-engine switch variants
    (32768, 128, 128, "gelu", False, ("rowpanel",)),                 # exactly 256 rounds of 128 rows, no tail
    (32769, 384, 256, None, True, ("rowpanel",)),                    # 1-row tail
    (32768 + 127, 1024, 128, "silu", True, ("rowpanel",)),           # 127-row tail, N = 1024
    (65536 + 128 * 5 + 77, 256, 256, "gelu", True, ("rowpanel", "panel")),   # NS-bench-like M, 77-row tail
    (32768 + 200, 192, 96, "tanh", True, ("panel",)),                # panel: 128 blocks x 2 column tiles = 256, 200-row tail
    (32767, 192, 96, "sigmoid", False, ()),                          # 127 x 2 = 254 tiles: just below the panel threshold
    (24448, 256, 128, "softplus", True, ("small",)),                 # 191 x 2 = 382 tiles: small split, M % 256 == 128
    (24576, 256, 128, "ELU", False, ("small",)),                     # 384 tiles: exact kernel
    (4096, 256, 256, "gelu", True, ("small",)),                      # small split, M % 256 == 0
    (200, 64, 64, "relu", True, ()),                                 # M < 256
    (1000, 96, 12, None, True, ()),                                  # K % 32 != 0
    (333, 128, 76, "silu", False, ()),                               # K % 32 != 0, ragged M
]
_VARIANTS = {"rowpanel": dict(PA2D_LIN_ROWPANEL="off"), "panel": dict(PA2D_LIN_ROWPANEL="off", PA2D_LIN_PANEL="off"),
             "small": dict(PA2D_LIN_SMALL_SPLIT="off")}


@pytest.mark.parametrize("M,N,K,act,with_res,variants", LIN_CASES)
def test_linear_elementwise(kernel_env, M, N, K, act, with_res, variants):
    from transformerbasednavierstokesolver_amd import ops
    rng = np.random.default_rng(M + 3 * N + 7 * K)
    x0, w, b = _r(rng, M, K), _r(rng, N, K, scale=K ** -0.5), 0.1 * _r(rng, N)
    res0, dy0, pre20, dy20 = _r(rng, M, N), _r(rng, M, N), _r(rng, M, K), _r(rng, M, K)
    wd, bd = w.double(), b.double()
    runs = [("f32", {}), ("split", {})] + [("split", _VARIANTS[v]) for v in variants]
    if N % 32 == 0 and K % 32 == 0:
        runs.append(("bf16s", {}))
    refs = {}
    for engine, env in runs:
        _set_env(kernel_env, **env)
        tag = f"linear M={M} N={N} K={K} act={act} res={with_res} {env or 'default'}"
        key = "bf" if engine == "bf16s" else "f"
        eng = None if engine == "bf16s" else engine
        (x, xd), (res, resd), (dy, dyd) = (_store(t, engine) for t in (x0, res0, dy0))
        (pre2, pre2d), (dy2, dy2d) = (_store(t, engine) for t in (pre20, dy20))
        if key not in refs:      # fp64 references (the bf16-storage ones on the bf16 values the kernels see)
            lin, lin_abs = xd @ wd.t() + bd, xd.abs() @ wd.abs().t() + bd.abs()
            r = dict(pre=lin, pre_s=lin_abs)
            if act:
                a, da = _act_and_grad(act, lin)
                _, da2 = _act_and_grad(act, pre2d)
            else:
                a, da, da2 = lin, None, torch.ones_like(pre2d)
            r["y"] = a + (resd if with_res else 0)
            r["y_s"] = 1.13 * lin_abs + a.abs() + (resd.abs() if with_res else 0)   # |act'| <= 1.13 + act's own rounding
            g = dyd @ wd
            # act' is evaluated to an absolute (not relative) accuracy: where it crosses zero the product keeps |g| * ulp(1)
            r["dx"], r["dx_s"] = g * da2, (dyd.abs() @ wd.abs()) * da2.abs().clamp_min(1.0)
            r["dw"], r["dw_s"] = dyd.t() @ xd, dyd.abs().t() @ xd.abs()
            r["db"], r["db_s"] = dyd.sum(0), dyd.abs().sum(0)
            refs[key] = r
        r = refs[key]
        y, pre = poisoned(ops.linear_fwd, x, w, b, res=res if with_res else None, act=act, want_pre=True, engine=eng)
        _prod(pre, r["pre"], r["pre_s"], engine, "fwd", tag + " pre-activation")
        _prod(y, r["y"], r["y_s"], engine, "fwd", tag + " output")
        tol_f, tol_b = (BF_TOL, BF_TOL) if engine == "bf16s" else (FWD_TOL, BWD_TOL)
        assert rel_l2(y, r["y"]) < tol_f and rel_l2(pre, r["pre"]) < tol_f
        dx = poisoned(ops.linear_bwd_data, dy, w, pre=pre2 if act else None, act=act, engine=eng)
        _prod(dx, r["dx"], r["dx_s"], engine, "fwd", tag + " data gradient")
        assert rel_l2(dx, r["dx"]) < tol_b
        dw, db = poisoned(ops.linear_bwd_weight, dy, x, engine=eng)
        _prod(dw, r["dw"], r["dw_s"], engine, "wgrad", tag + " weight gradient")
        _prod(db, r["db"], r["db_s"], engine, "wgrad", tag + " bias gradient")
        assert rel_l2(dw, r["dw"]) < (1e-4 if engine == "bf16s" else BWD_TOL) and rel_l2(db, r["db"]) < 1e-4
        if act:      # MODE 2: the forward saves act'(pre-activation), the data gradient multiplies by it
            y2, d = poisoned(ops.linear_fwd, x, w, b, res=res if with_res else None, act=act, want_pre=True, engine=eng,
                             save_derivative=True)
            assert torch.equal(y2, y)
            # act'(pre-activation) as the epilogue evaluates it, against fp64 act' of the pre-activation the kernel stored
            _, da_k = _act_and_grad(act, pre.double())
            _prod(d, da_k, 1.0 + pre.double().abs(), engine, "fwd", tag + " saved derivative")
            wt = w.t().contiguous()        # dx2 [M, N] = (dy2 [M, K] . w^T) * d, d [M, N]
            dx2 = poisoned(ops.linear_bwd_data, dy2, wt, pre=d, act=act, engine=eng, pre_is_derivative=True)
            dd = d.double()
            g2 = dy2d @ wd.t()
            _prod(dx2, g2 * dd, (dy2d.abs() @ wd.abs().t()) * dd.abs(), engine, "fwd",
                  tag + " data gradient (saved derivative)")
            assert rel_l2(dx2, g2 * dd) < tol_b
    _set_env(kernel_env)


# ---------------------------------------------------------------------------------------------- conv 3x3 x 2
def _conv(x, w, b, H, W):
    """Zero-padded 3x3 cross-correlation (oracle.conv3x3) as nine shifted GEMMs: fp64 on the device."""
    B, N, C = x.shape
    xp = F.pad(x.reshape(B, H, W, C), (0, 0, 1, 1, 1, 1))
    out = b.expand(B, H, W, w.shape[0])
    for ky in range(3):
        for kx in range(3):
            out = out + xp[:, ky:ky + H, kx:kx + W, :] @ w[:, :, ky, kx].t()
    return out.reshape(B, N, -1)


def _conv_refs(x, wx, bx, wf, bf, dout, H, W):
    """(out, dxn, dwx, dbx, dwf, dbf) of the fused pair, and the same on absolute values (the scales)."""
    def run(x, wx, bx, wf, bf, dout):
        ts = [t.detach().clone().requires_grad_(True) for t in (x, wx, bx, wf, bf)]
        out = torch.cat([_conv(ts[0], ts[1], ts[2], H, W), _conv(ts[0], ts[3], ts[4], H, W)], -1)
        out.backward(dout)
        return (out.detach(),) + tuple(t.grad for t in ts)
    ref = run(x, wx, bx, wf, bf, dout)
    scale = run(x.abs(), wx.abs(), bx.abs(), wf.abs(), bf.abs(), dout.abs())
    return ref, scale


CONV_CASES = [  # B, H, W, C, [(engine, env), ...]
    (2, 64, 64, 256, [("split", {}), ("split", dict(PA2D_CONV_MFMA="32")), ("split", dict(PA2D_MC_BIG="off")),
                      ("split", dict(PA2D_CONV_HALO="off")), ("f32", {}), ("bf16s", {})]),
    (1, 45, 70, 64, [("split", dict(PA2D_CONV_HALO="force")), ("split", dict(PA2D_CONV_HALO="force", PA2D_CONV_MFMA="32")),
                     ("split", dict(PA2D_CONV_HALO="off", PA2D_MC_BIG="off")), ("bf16s", dict(PA2D_CONV_HALO="force")),
                     ("bf16s", dict(PA2D_CONV_HALO="off"))]),
    (2, 128, 128, 256, [("split", dict(PA2D_CONV_HALO="off"))]),           # split_big: M % 256 == 0, 512 tiles
    (1, 127, 256, 256, [("split", dict(PA2D_CONV_HALO="off"))]),           # 508 tiles: 128x128
    (2, 130, 129, 256, [("split", dict(PA2D_CONV_HALO="off"))]),           # M % 256 != 0
    (1, 12, 20, 64, [("split", {}), ("f32", {}), ("bf16s", {})]),           # M = 240 < 256: 64-row tiles
    (1, 20, 24, 48, [("split", {}), ("f32", {})]),                          # Cin % 32 != 0: exact kernel, 16-wide K-step
    (1, 421, 421, 128, [("split", {}), ("split", dict(PA2D_CONV_MFMA="32")), ("bf16s", {})]),   # Darcy, B = 1
]


@pytest.mark.parametrize("B,H,W,C,runs", CONV_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}x{c[3]}" for c in CONV_CASES])
def test_conv_elementwise(kernel_env, B, H, W, C, runs):
    from transformerbasednavierstokesolver_amd import ops
    rng = np.random.default_rng(B * H + W + C)
    N = H * W
    x0, dout0 = _r(rng, B, N, C), _r(rng, B, N, 2 * C)
    wx, wf = _r(rng, C, C, 3, 3, scale=(9 * C) ** -0.5), _r(rng, C, C, 3, 3, scale=(9 * C) ** -0.5)
    bx, bf = 0.1 * _r(rng, C), 0.1 * _r(rng, C)
    refs = {}
    for engine, env in runs:
        _set_env(kernel_env, **env)
        tag = f"conv B={B} H={H} W={W} C={C} {env or 'default'}"
        key = "bf" if engine == "bf16s" else "f"
        eng = None if engine == "bf16s" else engine
        (x, xd), (dout, doutd) = _store(x0, engine), _store(dout0, engine)
        if key not in refs:
            refs[key] = _conv_refs(xd, wx.double(), bx.double(), wf.double(), bf.double(), doutd, H, W)
        (out_r, dx_r, dwx_r, dbx_r, dwf_r, dbf_r), (out_s, dx_s, dwx_s, dbx_s, dwf_s, dbf_s) = refs[key]
        out = poisoned(ops.conv3x3x2_fwd, x, wx, bx, wf, bf, H, W, engine=eng)
        _prod(out, out_r, out_s, engine, "fwd", tag + " forward", hw=(H, W))
        tol_f, tol_b = (BF_TOL, BF_TOL) if engine == "bf16s" else (FWD_TOL, BWD_TOL)
        assert rel_l2(out, out_r) < tol_f
        dxn, dwx, dbx, dwf, dbf = poisoned(ops.conv3x3x2_bwd, dout, x, wx, wf, H, W, engine=eng)
        _prod(dxn, dx_r, dx_s, engine, "fwd", tag + " data gradient", hw=(H, W))
        for got, ref, sc, name in ((dwx, dwx_r, dwx_s, "dwx"), (dwf, dwf_r, dwf_s, "dwf")):
            _prod(got.reshape(C, -1), ref.reshape(C, -1), sc.reshape(C, -1), engine, "wgrad", f"{tag} {name} [co, ci*9+tap]")
        _prod(dbx, dbx_r, dbx_s, engine, "wgrad", tag + " dbx")
        _prod(dbf, dbf_r, dbf_s, engine, "wgrad", tag + " dbf")
        assert rel_l2(dxn, dx_r) < tol_b
        tol_w = 1e-4 if engine == "bf16s" else BWD_TOL
        assert rel_l2(dwx, dwx_r) < tol_w and rel_l2(dwf, dwf_r) < tol_w
        assert rel_l2(dbx, dbx_r) < tol_w and rel_l2(dbf, dbf_r) < tol_w
    _set_env(kernel_env)


# ---------------------------------------------------------------------------------------------- slice path
SLICE_CASES = [  # B, N, heads, D, M: N never a multiple of 32 or of the points-per-chunk
    (2, 1037, 4, 8, 12),
    (2, 4096 + 17, 8, 32, 64),      # NS bench geometry (B = 2), ragged N
    (1, 4100, 8, 16, 128),          # Darcy kernels: M = 128, D = 16
    (1, 3001, 2, 16, 64),
]


def _slice_refs(xf, dy, ws, bs, temp, wq, wk, wv, heads):
    """fp64 on the device: forward (oracle), backward (oracle.slice_core_backward) and the absolute-value scales."""
    from oracle import transolver_oracle as orc
    B, N, C2 = xf.shape
    C = C2 // 2
    D = C // heads
    xm, fm = xf[..., :C], xf[..., C:]
    w, norm, s, tok = orc.slice_tokens(xm, fm, ws, bs, temp, heads)
    o = orc.token_attention(tok, wq, wk, wv)
    y = orc.deslice(w, o)
    bw = orc.slice_core_backward(xm, fm, dy, ws, bs, temp, wq, wk, wv, heads)
    fh, xh, dyh = orc.split_heads(fm, heads), orc.split_heads(xm, heads), orc.split_heads(dy, heads)
    tau = temp.reshape(1, -1, 1, 1).clamp(orc.TAU_MIN, orc.TAU_MAX)
    logit = (xh @ ws.t() + bs) / tau
    # |dL/dlogit| bound: dW = dY O^T + F dS^T + dn on absolute values, through the softmax Jacobian on absolute values
    dw_abs = dyh.abs() @ o.abs().transpose(-1, -2) + fh.abs() @ bw["ds"].abs().transpose(-1, -2) + bw["dn"].abs()[:, :, None, :]
    dl_abs = w * (dw_abs + (dw_abs * w).sum(-1, keepdim=True))
    merge = lambda z: z.permute(0, 2, 1, 3).reshape(B, N, C)
    sc = dict(
        s=w.transpose(-1, -2) @ fh.abs(), norm=norm, do=w.transpose(-1, -2) @ dyh.abs(),
        dxm=merge((dl_abs @ ws.abs()) / tau), dfm=merge(w @ bw["ds"].abs()),
        y=orc.deslice(w, o.abs()),
        dws=((dl_abs / tau).transpose(-1, -2) @ xh.abs()).sum((0, 1)),
        dbs=(dl_abs / tau).sum((0, 1, 2)),
        dtemp=((dl_abs * logit.abs()).sum((0, 2, 3)) / tau.reshape(-1)),
    )
    return dict(s=s, norm=norm, o=o, y=y, **bw), sc


@pytest.mark.parametrize("B,N,heads,D,M", SLICE_CASES)
def test_slice_elementwise(B, N, heads, D, M):
    from transformerbasednavierstokesolver_amd import ops
    C = heads * D
    rng = np.random.default_rng(B + N + M + D)
    xf0, dy0 = _r(rng, B, N, 2 * C), _r(rng, B, N, C)
    ws, bs = _r(rng, M, D, scale=D ** -0.5), 0.3 * _r(rng, M)
    temp = torch.tensor(np.resize(np.array([0.03, 0.5, 7.0, 0.25, 1.5, 0.1, 5.0, 0.8], dtype=np.float32), heads)).to(DEV)
    wq, wk, wv = (_r(rng, D, D, scale=1.5 * D ** -0.5) for _ in range(3))
    d = lambda t: t.double()
    f32 = lambda t, *shape: t.float().reshape(*shape).contiguous()
    refs = {}
    for engine in ("f32", "split", "bf16s"):
        tag = f"slice B={B} N={N} heads={heads} D={D} M={M}"
        key = "bf" if engine == "bf16s" else "f"
        eng = None if engine == "bf16s" else engine
        (xf, xfd), (dy, dyd) = _store(xf0, engine), _store(dy0, engine)
        if key not in refs:
            refs[key] = _slice_refs(xfd, dyd, d(ws), d(bs), d(temp), d(wq), d(wk), d(wv), heads)
        r, sc = refs[key]
        tol_f, tol_b = (BF_TOL, BF_TOL) if engine == "bf16s" else (FWD_TOL, BWD_TOL)
        # scatter: raw sums S and norms, summed over the point chunks in fp64
        spart, npart = poisoned(ops.slice_scatter, xf, 2 * C, 0, xf, 2 * C, C, ws, bs, temp, B, N, heads, D, M, engine=eng)
        s_k = spart.double().sum(1).view(B, heads, M, D)
        n_k = npart.double().sum(1).view(B, heads, M)
        _prod(s_k, r["s"], sc["s"], engine, "slice", tag + " scatter S [b, h, m, d]")
        _prod(n_k, r["norm"], sc["norm"], engine, "slice", tag + " scatter norm [b, h, m]")
        assert rel_l2(s_k, r["s"]) < FWD_TOL if engine != "bf16s" else rel_l2(s_k, r["s"]) < BF_TOL
        # token attention: per token
        s2, nrm, o = poisoned(ops.token_attn_fwd, spart, npart, wq, wk, wv)
        _rows(o.view(B * heads * M, D), r["o"].reshape(-1, D), engine, tag + " token attention O [token, d]")
        assert rel_l2(o.view(B, heads, M, D), r["o"]) < 2e-5 or engine == "bf16s"
        # de-slice with the oracle's tokens
        o_ref = f32(r["o"], B * heads, M, D)
        y = poisoned(ops.deslice_fwd, xf, 2 * C, 0, o_ref, ws, bs, temp, B, N, heads, D, M, engine=eng)
        _prod(y, r["y"], sc["y"], engine, "slice", tag + " de-slice Y [b, n, c]")
        assert rel_l2(y, r["y"]) < tol_f
        # backward: dO partials (element-wise), token attention backward (per token), point / parameter gradients
        dopart, _ = poisoned(ops.slice_scatter, xf, 2 * C, 0, dy, C, 0, ws, bs, temp, B, N, heads, D, M, want_norm=False,
                             engine=eng)
        _prod(dopart.double().sum(1).view(B, heads, M, D), r["do"], sc["do"], engine, "slice", tag + " dO [b, h, m, d]")
        ds, dn, dwq, dwk, dwv = poisoned(ops.token_attn_bwd, s2, nrm, wq, wk, wv, dopart)
        _rows(ds.view(-1, D), r["ds"].reshape(-1, D), engine, tag + " dS [token, d]")
        _rows(dn.view(B * heads, M), r["dn"].reshape(-1, M), engine, tag + " dn [b*h, m]")
        dxf, dws, dbs, dtemp = poisoned(ops.slice_bwd_points, xf, dy, ws, bs, temp, o_ref, f32(r["ds"], B * heads, M, D),
                                        f32(r["dn"], B * heads, M), B, N, heads, D, M, engine=eng)
        _prod(dxf[..., :C], r["dxm"], sc["dxm"], engine, "slice", tag + " dx_mid [b, n, c]")
        _prod(dxf[..., C:], r["dfm"], sc["dfm"], engine, "slice", tag + " dfx_mid [b, n, c]")
        _prod(dws, r["dws"], sc["dws"], engine, "slice", tag + " dws [m, d]")
        _prod(dbs, r["dbs"], sc["dbs"], engine, "slice", tag + " dbs [m]")
        _prod(dtemp, r["dtemperature"].reshape(heads), sc["dtemp"], engine, "slice", tag + " dtemperature [h]")
        assert rel_l2(dxf[..., :C], r["dxm"]) < tol_b and rel_l2(dxf[..., C:], r["dfm"]) < tol_b
        if engine != "bf16s":
            assert rel_l2(dws, r["dws"]) < BWD_TOL and rel_l2(dbs, r["dbs"]) < BWD_TOL


# ---------------------------------------------------------------------------------------------- LayerNorm, head
@pytest.mark.parametrize("rows,C", [(7, 32), (300, 64), (4096, 256), (1000, 1024), (66253, 256)])
def test_layernorm_elementwise(rows, C):
    from transformerbasednavierstokesolver_amd import ops
    from oracle import transolver_oracle as orc
    rng = np.random.default_rng(rows + C)
    x0, dy0, dres0 = _r(rng, rows, C) * 2 + 0.5, _r(rng, rows, C), _r(rng, rows, C)
    g, b = 1 + 0.1 * _r(rng, C), 0.1 * _r(rng, C)
    for engine in ("f32", "bf16s"):
        tag = f"layernorm rows={rows} C={C}"
        (x, xd), (dy, dyd), (dres, dresd) = (_store(t, engine) for t in (x0, dy0, dres0))
        xq = xd.clone().requires_grad_(True)
        gd, bd = g.double().requires_grad_(True), b.double().requires_grad_(True)
        yo = orc.layer_norm(xq, gd, bd)
        yo.backward(dyd)
        y, mean, rstd = poisoned(ops.layernorm_fwd, x, g, b)
        _rows(y, yo.detach(), engine, tag + " forward")
        dx, dg, db = poisoned(ops.layernorm_bwd, dy, x, mean, rstd, g, dres)
        _rows(dx, xq.grad + dresd, engine, tag + " dx")
        xhat = (yo.detach() - bd.detach()) / gd.detach()
        _prod(dg, gd.grad, (dyd.abs() * xhat.abs()).sum(0), "f32" if engine == "bf16s" else engine, "wgrad", tag + " dgamma")
        _prod(db, bd.grad, dyd.abs().sum(0), "f32" if engine == "bf16s" else engine, "wgrad", tag + " dbeta")
        tol = BF_TOL if engine == "bf16s" else FWD_TOL
        assert rel_l2(y, yo) < tol and rel_l2(dx, xq.grad + dresd) < (BF_TOL if engine == "bf16s" else BWD_TOL)


@pytest.mark.parametrize("rows,C,O", [(30, 32, 2), (4096, 256, 1), (500, 64, 5), (66253, 256, 1)])
def test_head_elementwise(rows, C, O):
    from transformerbasednavierstokesolver_amd import ops
    rng = np.random.default_rng(rows + O)
    x0, w, b, dy = _r(rng, rows, C), _r(rng, O, C, scale=C ** -0.5), 0.1 * _r(rng, O), _r(rng, rows, O)
    wd, dyd = w.double(), dy.double()
    for engine in ("f32", "bf16s"):
        tag = f"head rows={rows} C={C} O={O}"
        x, xd = _store(x0, engine)
        y = poisoned(ops.head_fwd, x, w, b)
        ref = xd @ wd.t() + b.double()
        # the head output is fp32 on both storage types; bf16 storage rounds nothing but the input (exact in the reference)
        _prod(y, ref, xd.abs() @ wd.abs().t() + b.double().abs(), "f32", "fwd", f"[{engine}] {tag} forward")
        assert rel_l2(y, ref) < FWD_TOL
        dx, dw, db = poisoned(ops.head_bwd, dy, x, w)
        _prod(dx, dyd @ wd, dyd.abs() @ wd.abs(), "f32", "fwd", f"[{engine}] {tag} dx")
        _prod(dw, dyd.t() @ xd, dyd.abs().t() @ xd.abs(), "f32", "wgrad", f"[{engine}] {tag} dw")
        _prod(db, dyd.sum(0), dyd.abs().sum(0), "f32", "wgrad", f"[{engine}] {tag} db")
        assert rel_l2(dx, dyd @ wd) < (BF_TOL if engine == "bf16s" else BWD_TOL)
