"""Element-wise fp64 parity of the operand-planes route: the producers that write a conv operand ONLY as a bf16 plane image
(layernorm_fwd_planes, slice_bwd_points_planes + the conv bias gradients) and the consumers that read such images
(conv3x3x2_fwd_planes, conv3x3x2_bwd_planes).  No fp32 copy of those tensors exists on this route, so every case checks

* the image itself: `check_canonical_planes` (bit for bit the hi / mid / lo split of the value it holds: swapped planes, a
  plane in the wrong slot and a stale plane fail whatever their sum) after a run through `poisoned` (the image is returned
  as a bf16 view, so the NaN sentinel of an unwritten element counts);
* the values: the plane sums against the fp64 references of tests/test_gpu_elementwise.py (`_slice_refs`, `_conv_refs`,
  the oracle's LayerNorm), element by element, under the bounds of elementwise_check.py (TAU / ROW_TOL): no new number;
* the consumers on images made by `to_planes` (plain torch), so that they do not depend on the producers: references on
  the fp64 plane sums, exactly the values the kernels read.

Geometries (engine "split": 3 planes, engine "bf16": 1 plane; conv_planes_mask == 7 for all of them):

    id  B, H, W     C, heads, D, M     reaches
    A   1, 23, 29   128, 8, 16, 128    v3 slice backward, K16 path, MT = 8 (Darcy); ragged N = 667; W < the halo tile's 32
    B   2, 19, 27   256, 8, 32, 128    exact-fp32 slice backward writing planes (slice_bwd3_built(32, 8) is false); two
                                       images; N = 513: the last group of a chunk holds one point
    C   1, 17, 19   128, 16, 8, 32     four heads per 32-channel chunk; 323 rows < 512: 128 x 128 planes weight gradient
    D   1, 25, 33   160, 5, 32, 64     5 / 10 chunks per row (dF starts at chunk 5); C % 64 != 0; 256-tiles ragged both ways
                                       (Mi = 320, Nj = 1440); second tile column one pixel wide; the v3 writer's 16-byte
                                       (lane-pair swap) stores
    E   3, 9, 31    192, 3, 64, 64     D = 64: slice_bwd3_built(64, 4) is true (LDS 111.5 KiB), so the v3 kernel writes, with
                                       the 8-byte stores of its general path (DT = 4); tiles that end at image boundaries

Which slice-backward kernel writes the image decides the bound: TAU[("split", "slice")] for the v3 kernel,
TAU[("f32", "slice")] for the exact-fp32 one (case B), + 2^-8 |ref| for the one-plane image (one rounding of the stored
value).  Conv consumers: TAU[("split", "fwd" | "wgrad")] for 3 planes, TAU[("bf16s", "fwd" | "wgrad")] without the 2^-8
term for 1 plane (fp32 outputs, activations exact in bf16, only the weights rounded in the kernel).  LayerNorm rows:
ROW_TOL["f32"] / ROW_TOL["bf16s"], the bounds of the fp32-stored / bf16-stored LayerNorm output.  Accumulating calls
(`into=`) start from random buffers of the gradients' magnitude; got - prefill meets the same bound with
(2^-24 / tau) (|prefill| + |ref|), one fp32 addition, added to the scale.

Arms of the consumers (kernel_env): default (per-tile conv gemm_kc_split_kernel with pre-split A; 256 x 256 planes weight
gradient, 128 x 128 at case C), PA2D_CONV_HALO=force (conv_halo_kernel, 16x16x32), + PA2D_CONV_MFMA=32 (32x32x16),
PA2D_MC_MFMA=32, PA2D_MC_BIG=off (128 x 128 planes kernel at A, B, C; at D and E the mask drops below 7 and the backward
entry point refuses).

Block: functional.attn_branch, split engine (planes route, asserted) against engine f32 (fp32 route), gradients added into
a FlatGradSync bucket as the models do; a second backward must double every parameter gradient.  At A the whole block
runs.  At B (M = 128, D = 32) no engine has a token-attention backward (its LDS need, 205 KiB, passes 160 KiB:
pa2d_token_attn_bwd returns "unsupported"), so a model of that geometry cannot train on any route: the case checks the
forward on the planes route and that the backward refuses.  B96 (B with M = 96, the largest multiple of 16 whose token
backward fits) is the block that does train through the exact-fp32 plane writer; it also runs in the slice-backward cases
(M < the kernel's padded 128 slices).

KERNEL COVERAGE (one rocprofv3 --kernel-trace --stats run over this file alone, MI355X; launches in brackets):

    LayerNorm        layernorm_fwd_planes_kernel<3> [17], <1> [12]
    slice backward   slice_bwd3_kernel<16, 8, float, 3 | 1> (A), <32, 4, float, 3 | 1> (D), <64, 4, float, 3 | 1> (E),
                     <8, 2, float, 3 | 1> (C): the v3 writer [32 in all]
                     slice_bwd_kernel<32, 8, float, 3> [11], <32, 8, float, 1> [9] (B, B96): the exact-fp32 writer
                     conv_bias_finalize_kernel [52], dtau_finalize_kernel, reduce_segs_kernel
    conv             conv_halo_kernel<3, float, 1, true> (16x16x32) [20], <3, float, 1, false> (32x32x16) [20],
                     <1, float, 3, false> [40]
                     gemm_kc_split_kernel<64, 128, true, 3, true, float, 9> [85], <128, 128, true, 1, true, float, 9> [71]:
                     the per-tile conv on a pre-split A
    weight gradient  gemm_mc_planes_big_kernel<3, 1, true> [44], <3, 1, false> (PA2D_MC_MFMA=32) [8], <1, 4, false> [48]
                     gemm_mc_planes_kernel<3, 1, false, false> [17], <1, 4, false, false> [17]; reduce_slabs_kernel<9>
    block            + token_attn_fwd / _bwd, the fp32 route's slice_bwd_kernel<.., 0>, split_planes_kernel, gemm_mc_kernel

CALIBRATION (MI355X, the module's end-of-run report, pytest -s: worst |got - ref| / scale, rows: per-row rel-L2):

    image     family  worst     bound                          worst case
    3 planes  rows    1.4e-7    ROW_TOL["f32"] 1.9e-5          LayerNorm A (E 1.4e-7, B 1.3e-7)
    1 plane   rows    2.2e-3    ROW_TOL["bf16s"] 9e-3          LayerNorm A (E, C 2.1e-3)
    3 planes  slice   5.5e-6    TAU[("split", "slice")] 1e-5   v3 writer, A dfx_mid (D 2.9e-6, C 2.4e-6)
    3 planes  slice   1.035e-5  TAU_V3_D64 2.2e-5              v3 writer, E dfx_mid; sibling slice_bwd_points(engine="split"):
                                                               1.035e-5, the same values bit for bit (engine f32: 1.65e-5)
    3 planes  slice   1.06e-5   TAU[("f32", "slice")] 2e-5     exact writer, chain B dfx_mid (B96 8.8e-6, B 8.7e-6)
    1 plane   slice   2.6e-6    2e-5 + 2^-8 |ref|              exact writer, chain B dfx_mid (v3 writer: 1.6e-7 under 1e-5)
    3 planes  fwd     7.6e-7    TAU[("split", "fwd")] 1.6e-6   chain B data gradient (conv forward: 3.0e-7)
    3 planes  wgrad   1.5e-7    TAU[("split", "wgrad")] 1e-6   conv C dwx, every arm
    1 plane   fwd     7.9e-4    TAU[("bf16s", "fwd")] 5e-3     chain A data gradient (forward 4.3e-4)
    1 plane   wgrad   8.1e-8    TAU[("bf16s", "wgrad")] 3e-7   chain B dwf
    block     rel-L2  3.0e-6    1e-5                           B96 wx, split (planes route) against f32 (A: 2.5e-6, temperature)

In every 3-plane case of the slice backward the image holds exactly the values the sibling fp32-tensor op writes.

Spot check (a scratch build, not part of the tree): with the mid and lo plane stores of slice_bwd_kernel<.., PL> exchanged,
test_slice_bwd_planes[split-3-B], [split-3-B96] and test_planes_chain[split-3-B] fail in check_canonical_planes (525302 of
525312 elements, planes [1, 2]); the conv backward fed that image gives 1.9e-6 (data gradient), 2.4e-6 (dwx), 1.4e-6
(dwf), over TAU[("split", "fwd")] = 1.6e-6 and TAU[("split", "wgrad")] = 1e-6 (clean: 7.6e-7, 1.3e-7, 1.3e-7); the block's
rel-L2 1e-5 and test_operand_planes_interface do not see it.
"""
import numpy as np
import pytest
import torch

from conftest import rel_l2
from elementwise_check import (BF16_STORAGE_REL, ROW_TOL, TAU, check_canonical_planes, check_products, check_rows, poisoned,
                               to_planes, unplane)
from test_gpu_elementwise import DEV, _conv_refs, _note, _r, _report, _slice_refs  # noqa: F401  (_report prints the WORST table)

pytestmark = pytest.mark.gpu
ENV_KEYS = ("PA2D_CONV_HALO", "PA2D_CONV_MFMA", "PA2D_MC_MFMA", "PA2D_MC_BIG")
# Point gradients [dX | dF] of the v3 slice backward at D = 64 (case E): a new worst case of the ("split", "slice") family, not a
# planes matter.  The sibling fp32-tensor op slice_bwd_points(engine="split") on the same inputs reaches 1.035e-5 on dfx_mid
# (one element of 160704 above TAU[("split", "slice")] = 1e-5; the exact-fp32 kernel: 1.65e-5 under its 2e-5), and the image
# holds the same values bit for bit.  Bound <= 4 x the sibling's worst, with the headroom of the TAU entries (2.2 x).
TAU_V3_D64 = 2.2e-5

GEOM = {  # id: B, H, W, C, heads, D, M, exact (the slice backward that writes planes is the exact-fp32 kernel)
    "A": (1, 23, 29, 128, 8, 16, 128, False),
    "B": (2, 19, 27, 256, 8, 32, 128, True),
    "C": (1, 17, 19, 128, 16, 8, 32, False),
    "D": (1, 25, 33, 160, 5, 32, 64, False),
    "E": (3, 9, 31, 192, 3, 64, 64, False),
    "B96": (2, 19, 27, 256, 8, 32, 96, True),      # slice backward and block only, see the docstring
}
ENGINES = [("split", 3), ("bf16", 1)]
ARMS = [{}, dict(PA2D_CONV_HALO="force"), dict(PA2D_CONV_HALO="force", PA2D_CONV_MFMA="32"), dict(PA2D_MC_MFMA="32"),
        dict(PA2D_MC_BIG="off")]
cases = pytest.mark.parametrize("gid", ["A", "B", "C", "D", "E"])
engines = pytest.mark.parametrize("engine,nt", ENGINES)


def _set_env(kernel_env, **kv):
    kernel_env(**{k: kv.get(k) for k in ENV_KEYS})


def _rec(nt):
    return f"plane{nt}"      # the engine column of the WORST table


def _prod(got, ref, scale, tau_key, nt, label, *, rel_ref=0.0, hw=None, tau=None):
    """`tau`: a bound of this module that stands in for TAU[tau_key] (TAU_V3_D64)"""
    v = check_products(got, ref, scale, tau or TAU[tau_key], rel_ref=rel_ref, hw=hw, label=f"[{nt} planes] {label}")
    _note(_rec(nt), tau_key[1], f"{label} ({f'tau {tau:.3g}' if tau else f'TAU[{tau_key}]'})", v)


def _acc(got, pre, ref, scale, tau_key, nt, label):
    """got = pre + gradient: the gradient's bound, widened by the one fp32 addition that made `got`."""
    tau = TAU[tau_key]
    sc = scale + (2.0 ** -24 / tau) * (pre.double().abs() + ref.abs())
    check_products(got.double() - pre.double(), ref, sc, tau, label=f"[{nt} planes] {label} accumulated into a pre-filled buffer")


def _prefill(rng, ref):
    return _r(rng, *ref.shape, scale=float(ref.abs().mean()))


def _image(planes):
    """the uint8 image as a bf16 view: the NaN sentinel of `poisoned` counts"""
    return planes.view(torch.bfloat16)


def _tag(gid, engine):
    B, H, W, C, heads, D, M, exact = GEOM[gid]
    return f"{gid} {B}x{H}x{W} C={C} heads={heads} D={D} M={M} engine={engine}"


# ---------------------------------------------------------------------------------------------- producers
@cases
@engines
def test_layernorm_planes(kernel_env, gid, engine, nt):
    from transformerbasednavierstokesolver_amd import ops
    from oracle import transolver_oracle as orc
    _set_env(kernel_env)
    B, H, W, C, *_ = GEOM[gid]
    rows = B * H * W
    assert ops.conv_planes_mask(B, H, W, C, engine) == 7
    rng = np.random.default_rng(rows + C)
    x = _r(rng, rows, C) * 2 + 0.5
    g, b = 1 + 0.1 * _r(rng, C), 0.1 * _r(rng, C)
    tag = f"layernorm planes {_tag(gid, engine)}"
    yo = orc.layer_norm(x.double(), g.double(), b.double())
    img, mean, rstd = poisoned(lambda: (lambda p, m, r: (_image(p), m, r))(*ops.layernorm_fwd_planes(x, g, b, engine)))
    _, mean0, rstd0 = ops.layernorm_fwd(x, g, b)
    assert torch.equal(mean, mean0) and torch.equal(rstd, rstd0)
    total = check_canonical_planes(img, rows, C, nt, label=tag)
    v = check_rows(total, yo, ROW_TOL["f32" if nt == 3 else "bf16s"], label=tag)
    _note(_rec(nt), "rows", tag, v)


def _slice_inputs(gid):
    B, H, W, C, heads, D, M, exact = GEOM[gid]
    N = H * W
    rng = np.random.default_rng(B + N + M + D)
    xf, dy = _r(rng, B, N, 2 * C), _r(rng, B, N, C)
    ws, bs = _r(rng, M, D, scale=D ** -0.5), 0.3 * _r(rng, M)
    temp = torch.tensor(np.resize(np.array([0.03, 0.5, 7.0, 0.25, 1.5, 0.1, 5.0, 0.8], dtype=np.float32), heads)).to(DEV)
    wq, wk, wv = (_r(rng, D, D, scale=1.5 * D ** -0.5) for _ in range(3))
    return rng, xf, dy, ws, bs, temp, wq, wk, wv


def _slice_bwd_planes_checked(ops, rng, gid, engine, nt, xf, dy, ws, bs, temp, wq, wk, wv, tag):
    """slice_bwd_points_planes on upstream tensors from the oracle; every output checked; returns the image."""
    B, H, W, C, heads, D, M, exact = GEOM[gid]
    N = H * W
    d = lambda t: t.double()
    f32 = lambda t, *shape: t.float().reshape(*shape).contiguous()
    r, sc = _slice_refs(d(xf), d(dy), d(ws), d(bs), d(temp), d(wq), d(wk), d(wv), heads)
    spart, npart = ops.slice_scatter(xf, 2 * C, 0, xf, 2 * C, C, ws, bs, temp, B, N, heads, D, M, engine=engine)
    _, nrm, _ = ops.token_attn_fwd(spart, npart, wq, wk, wv)
    o, ds, dn = f32(r["o"], B * heads, M, D), f32(r["ds"], B * heads, M, D), f32(r["dn"], B * heads, M)
    args = (xf, dy, ws, bs, temp, o, ds, dn, nrm, B, N, heads, D, M, engine)
    img, dbx, dbf, dws, dbs, dtemp = poisoned(
        lambda: (lambda p, *rest: (_image(p),) + rest)(*ops.slice_bwd_points_planes(*args)))
    key = ("f32" if exact else "split", "slice")
    tag = f"{tag} ({'exact-fp32' if exact else 'v3'} writer)"
    total = check_canonical_planes(img, B * N, 2 * C, nt, label=tag).view(B, N, 2 * C)
    rel = BF16_STORAGE_REL if nt == 1 else 0.0
    pt_tau = TAU_V3_D64 if D == 64 and not exact else None
    _prod(total[..., :C], r["dxm"], sc["dxm"], key, nt, tag + " dx_mid [b, n, c]", rel_ref=rel, tau=pt_tau)
    _prod(total[..., C:], r["dfm"], sc["dfm"], key, nt, tag + " dfx_mid [b, n, c]", rel_ref=rel, tau=pt_tau)
    col = lambda t: t.sum((0, 1))
    grads = [(dbx, col(r["dxm"]), col(sc["dxm"]), "dbx [c]"), (dbf, col(r["dfm"]), col(sc["dfm"]), "dbf [c]"),
             (dws, r["dws"], sc["dws"], "dws [m, d]"), (dbs, r["dbs"], sc["dbs"], "dbs [m]"),
             (dtemp, r["dtemperature"].reshape(heads), sc["dtemp"], "dtemperature [h]")]
    for got, ref, scale, name in grads:
        _prod(got, ref, scale, key, nt, f"{tag} {name}")
    pre = tuple(_prefill(rng, ref) for _, ref, _, _ in grads)
    into = tuple(p.clone() for p in pre)
    img2, *_ = ops.slice_bwd_points_planes(*args, into=into)
    assert torch.equal(_image(img2), img)
    for got, p, (_, ref, scale, name) in zip(into, pre, grads):
        _acc(got, p, ref, scale, key, nt, f"{tag} {name}")
    return img


@pytest.mark.parametrize("gid", list(GEOM))
@engines
def test_slice_bwd_planes(kernel_env, gid, engine, nt):
    from transformerbasednavierstokesolver_amd import ops
    _set_env(kernel_env)
    B, H, W, C, *_ = GEOM[gid]
    assert ops.conv_planes_mask(B, H, W, C, engine) == 7
    rng, *inputs = _slice_inputs(gid)
    _slice_bwd_planes_checked(ops, rng, gid, engine, nt, *inputs, f"slice backward planes {_tag(gid, engine)}")


# ---------------------------------------------------------------------------------------------- consumers
def _conv_weights(rng, C):
    wx, wf = _r(rng, C, C, 3, 3, scale=(9 * C) ** -0.5), _r(rng, C, C, 3, 3, scale=(9 * C) ** -0.5)
    return wx, 0.1 * _r(rng, C), wf, 0.1 * _r(rng, C)


def _conv_fwd_checked(ops, gid, engine, nt, ximg, weights, refs, tag):
    B, H, W, C, *_ = GEOM[gid]
    (out_r, *_), (out_s, *_) = refs
    out = poisoned(ops.conv3x3x2_fwd_planes, ximg, *weights, B, H, W, engine)
    _prod(out, out_r, out_s, ("split" if nt == 3 else "bf16s", "fwd"), nt, tag + " forward", hw=(H, W))
    return out


def _conv_bwd_checked(ops, gid, engine, nt, dimg, ximg, weights, refs, tag, **kw):
    B, H, W, C, *_ = GEOM[gid]
    wx, _, wf, _ = weights
    (_, dx_r, dwx_r, _, dwf_r, _), (_, dx_s, dwx_s, _, dwf_s, _) = refs
    eng = "split" if nt == 3 else "bf16s"
    dxn, dwx, dwf = poisoned(ops.conv3x3x2_bwd_planes, dimg, ximg, wx, wf, B, H, W, engine, **kw)
    if kw.get("need_dx", True):
        _prod(dxn, dx_r, dx_s, (eng, "fwd"), nt, tag + " data gradient", hw=(H, W))
    else:
        assert dxn is None
    for got, ref, sc, name in ((dwx, dwx_r, dwx_s, "dwx"), (dwf, dwf_r, dwf_s, "dwf")):
        _prod(got.reshape(C, -1), ref.reshape(C, -1), sc.reshape(C, -1), (eng, "wgrad"), nt, f"{tag} {name} [co, ci*9+tap]")
    return dxn, dwx, dwf


@cases
@engines
def test_conv_planes(kernel_env, gid, engine, nt):
    from transformerbasednavierstokesolver_amd import ops
    B, H, W, C, *_ = GEOM[gid]
    N, rows = H * W, B * H * W
    rng = np.random.default_rng(B * H + W + C)
    ximg, dimg = to_planes(_r(rng, rows, C), nt), to_planes(_r(rng, rows, 2 * C), nt)
    weights = _conv_weights(rng, C)
    wx, bx, wf, bf = weights
    xs, ds = unplane(ximg, rows, C, nt)[1].view(B, N, C), unplane(dimg, rows, 2 * C, nt)[1].view(B, N, 2 * C)
    refs = _conv_refs(xs, wx.double(), bx.double(), wf.double(), bf.double(), ds, H, W)
    (_, _, dwx_r, _, dwf_r, _), (_, _, dwx_s, _, dwf_s, _) = refs
    for env in ARMS:
        _set_env(kernel_env, **env)
        tag = f"conv planes {_tag(gid, engine)} {env or 'default'}"
        mask = ops.conv_planes_mask(B, H, W, C, engine)
        out = _conv_fwd_checked(ops, gid, engine, nt, ximg, weights, refs, tag)
        if env.get("PA2D_MC_BIG") == "off" and C % 128:
            # no 128 x 128 planes weight gradient at this width: the route is refused as a whole, nothing comes back
            assert mask != 7 and mask & 1, mask
            with pytest.raises(RuntimeError, match="conv3x3x2_bwd_planes failed with code 1002"):
                ops.conv3x3x2_bwd_planes(dimg, ximg, wx, wf, B, H, W, engine)
            continue
        assert mask == 7, mask
        dxn, dwx, dwf = _conv_bwd_checked(ops, gid, engine, nt, dimg, ximg, weights, refs, tag)
        if env:
            continue
        # default arm only: the forward from planes == the forward that splits the same fp32 values itself (3 planes)
        if nt == 3:
            assert torch.equal(out, ops.conv3x3x2_fwd(xs.float(), wx, bx, wf, bf, H, W, engine=engine))
        # the weight gradients do not depend on whether the data gradient runs
        _, dwx2, dwf2 = _conv_bwd_checked(ops, gid, engine, nt, dimg, ximg, weights, refs, tag + " need_dx=False",
                                          need_dx=False)
        assert torch.equal(dwx2, dwx) and torch.equal(dwf2, dwf)
        # accumulate
        pre = (_prefill(rng, dwx_r), _prefill(rng, dwf_r))
        into = tuple(p.clone() for p in pre)
        dxn3, *_ = ops.conv3x3x2_bwd_planes(dimg, ximg, wx, wf, B, H, W, engine, into=into)
        assert torch.equal(dxn3, dxn)
        key = ("split" if nt == 3 else "bf16s", "wgrad")
        _acc(into[0].reshape(C, -1), pre[0].reshape(C, -1), dwx_r.reshape(C, -1), dwx_s.reshape(C, -1), key, nt, tag + " dwx")
        _acc(into[1].reshape(C, -1), pre[1].reshape(C, -1), dwf_r.reshape(C, -1), dwf_s.reshape(C, -1), key, nt, tag + " dwf")
    _set_env(kernel_env)


# ---------------------------------------------------------------------------------------------- chain
@pytest.mark.parametrize("gid", ["A", "B"])
@engines
def test_planes_chain(kernel_env, gid, engine, nt):
    """The producers' images go straight to the consumers, as functional.attn_forward / attn_backward pass them on; the
    consumers' references are taken on the producers' plane sums."""
    from transformerbasednavierstokesolver_amd import ops
    _set_env(kernel_env)
    B, H, W, C, heads, D, M, exact = GEOM[gid]
    N, rows = H * W, B * H * W
    assert ops.conv_planes_mask(B, H, W, C, engine) == 7
    rng, _, dy, ws, bs, temp, wq, wk, wv = _slice_inputs(gid)
    tag = f"chain {_tag(gid, engine)}"
    x = _r(rng, rows, C) * 2 + 0.5
    g, b = 1 + 0.1 * _r(rng, C), 0.1 * _r(rng, C)
    weights = _conv_weights(rng, C)
    ximg, _, _ = ops.layernorm_fwd_planes(x, g, b, engine)
    xs = check_canonical_planes(ximg, rows, C, nt, label=tag + " LayerNorm image").view(B, N, C)
    xf = ops.conv3x3x2_fwd_planes(ximg, *weights, B, H, W, engine)
    dimg = _slice_bwd_planes_checked(ops, rng, gid, engine, nt, xf, dy, ws, bs, temp, wq, wk, wv, tag + " slice backward")
    ds = unplane(dimg, rows, 2 * C, nt)[1].view(B, N, 2 * C)
    refs = _conv_refs(xs, *(t.double() for t in weights), ds, H, W)
    out = _conv_fwd_checked(ops, gid, engine, nt, ximg, weights, refs, tag)
    assert torch.equal(out, xf)
    _conv_bwd_checked(ops, gid, engine, nt, _image(dimg), ximg, weights, refs, tag)


# ---------------------------------------------------------------------------------------------- block
def _block_params(gid):
    B, H, W, C, heads, D, M, exact = GEOM[gid]
    rng = np.random.default_rng(7 * C + M)
    temp = torch.tensor(np.resize(np.array([0.5, 1.0, 0.7, 1.5, 0.4, 2.0, 0.9, 0.6], dtype=np.float32), heads))
    wx, bx, wf, bf = _conv_weights(rng, C)
    p = dict(ln_w=1 + 0.1 * _r(rng, C), ln_b=0.1 * _r(rng, C), temperature=temp.view(1, heads, 1, 1).to(DEV),
             wx=wx, bx=bx, wf=wf, bf=bf, ws=_r(rng, M, D, scale=D ** -0.5), bs=0.3 * _r(rng, M),
             wq=_r(rng, D, D, scale=D ** -0.5), wk=_r(rng, D, D, scale=D ** -0.5), wv=_r(rng, D, D, scale=D ** -0.5),
             wo=_r(rng, C, C, scale=C ** -0.5), bo=0.1 * _r(rng, C))
    return p, _r(rng, B, H * W, C), _r(rng, B, H * W, C)


@pytest.mark.parametrize("gid", ["A", "B", "B96"])
def test_attn_branch_planes_route(kernel_env, monkeypatch, gid):
    from transformerbasednavierstokesolver_amd import _lib, functional as Fn, ops
    from transformerbasednavierstokesolver_amd.ddp import FlatGradSync
    _set_env(kernel_env)
    B, H, W, C, heads, D, M, exact = GEOM[gid]
    # the token-attention backward keeps its operands in LDS: none is built for M = 128 with D = 32 (205 KiB), on any engine
    no_token_bwd = _lib.load().pa2d_token_attn_lds_bytes(M, D, 1) > 160 * 1024
    assert no_token_bwd == (gid == "B")
    p0, fx0, dout = _block_params(gid)
    calls = []
    for name in ("layernorm_fwd_planes", "conv3x3x2_fwd_planes", "slice_bwd_points_planes", "conv3x3x2_bwd_planes"):
        def spy(*a, _f=getattr(ops, name), _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, spy)
    res = {}
    for engine in ("split", "f32"):
        del calls[:]
        P = {k: v.clone().requires_grad_(True) for k, v in p0.items()}
        sync = FlatGradSync(P.values())           # before the backward: the kernels add straight into the bucket
        fx = fx0.clone().requires_grad_(True)
        run = lambda: Fn.attn_branch(fx, P["ln_w"], P["ln_b"], H, W, heads, [P[k] for k in Fn.ATTN_KEYS], engine=engine)
        out = run()
        assert ops.conv_planes_mask(B, H, W, C, engine) == (7 if engine == "split" else 0)
        assert calls == (["layernorm_fwd_planes", "conv3x3x2_fwd_planes"] if engine == "split" else [])
        res[engine] = dict(out=out.detach())
        if no_token_bwd:      # refused, not computed some other way
            with pytest.raises(RuntimeError, match="token_attn_bwd failed with code 1002"):
                out.backward(dout)
            continue
        out.backward(dout)
        torch.cuda.synchronize()
        assert calls[2:] == (["slice_bwd_points_planes", "conv3x3x2_bwd_planes"] if engine == "split" else [])
        assert all(P[k].grad.data_ptr() == sync.views[i].data_ptr() for i, k in enumerate(P))
        g1 = {k: v.grad.clone() for k, v in P.items()}
        res[engine].update(dfx=fx.grad.clone(), **g1)
        run().backward(dout)                      # accumulate adds, it does not overwrite
        for k, v in P.items():
            twice = 2 * g1[k].double()
            assert bool(((v.grad.double() - twice).abs() <= 2.0 ** -23 * twice.abs()).all()), (engine, k)
    assert set(res["split"]) == ({"out"} if no_token_bwd else {"out", "dfx", "ln_w", "ln_b"} | set(Fn.ATTN_KEYS))
    for k in res["split"]:
        e = rel_l2(res["split"][k], res["f32"][k])
        print(f"attn_branch {gid} split (planes route) vs f32: {k:12s} rel-L2 {e:.3e}")
        assert e < 1e-5, (k, e)
