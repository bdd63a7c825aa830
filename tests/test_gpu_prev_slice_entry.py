"""pa2d_prev_slice_entry_fwd / _bwd (csrc/pa2d_prev_slice.hip) element by element against fp64, in poisoned buffers.

    h0[b, n, :] = gelu( sw[b, n, :] . Wsw^T + tb[b, :] ),   dWsw = sum_rows dpre sw,   dtb[b] = sum_{rows of b} dpre

Bounds.
  forward   |got - ref| <= 1.13 tau (|sw| |Wsw|^T + |tb|) + R_GELU |ref|, tau = TAU[("f32", "fwd")] = 1.6e-6.  1.13 bounds
            the GELU slope: a rounding of the pre-activation reaches the output times at most that.  R_GELU is for
            gelu_exact's own error (the Abramowitz-Stegun erfc, |eps| <= 1.5e-7 absolute on Phi, plus two roundings).
  backward  |got - ref| <= tau_w S(|dpre|) + A_DGELU S(|dh0|), tau_w = TAU[("f32", "wgrad")] = 1e-6, dpre = dh0 gelu'(pre),
            S(v) = sum_rows v |sw| for dWsw and sum_{rows of b} v for dtb.  The first term is check_products' scale on the
            true |dpre|.  The second is for dgelu_exact, which holds gelu' to an ABSOLUTE accuracy (the erfc approximation's
            1.5e-7 on Phi, the rounding of the density term, and gelu'' times the rounding of the recomputed pre-activation):
            where gelu' is near 0 (x near -0.75) no multiple of |dpre| covers it.

Calibration of R_GELU and A_DGELU (MI355X, the four shapes below, every operand set, both routes): see the constants.

Operands that expose an indexing error: tb rows are offset by 1000 b (a wrong sample is off by ~1000); one run with
sw = 0 (the output is gelu(tb[b]) whatever Wsw is read); one run with the columns of Wsw scaled by 2^40 / 2^-40 alternately
(a wrong m pairs a weight with the wrong slice weight and is off by 2^80).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from elementwise_check import TAU, check_products, poisoned

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (B', N, M, C): H = 4 (M + M C)
SHAPES = [(1, 1, 1, 1),          # H = 8, a single row
          (3, 130, 4, 3),        # H = 64; several samples, N no multiple of a row chunk (64 forward, 128 backward)
          (5, 67, 64, 2),        # the largest M: four 16-column weight chunks
          (2, 4100, 16, 32)]     # the reference's H = 2112 = 33 * 64, no multiple of 128 or 256; N past 4096
# Worst (|got - ref| - 1.13 tau scale) / |ref| measured on the MI355X over the shapes and operand sets of this file:
# below zero everywhere (worst |got - ref| / (1.13 scale) = 7.1e-7 = 0.44 tau, at (5, 67, 64, 2) "plain"; 5.2e-7 at
# (2, 4100, 16, 32)): the first term alone holds every element, gelu_exact's error included, so nothing is added for it.
R_GELU = 0.0
# Worst max(0, |got - ref| - tau_w S(|dpre|)) / S(|dh0|) measured on the MI355X over the shapes, operand sets and routes of
# this file (kernel, three-op route, autograd to the layer's parameters): 2.35e-8, dtb at (5, 67, 64, 2) "sw0" (1.70e-8 on its
# "plain" set, 1.06e-8 at (3, 130, 4, 3) "sw0"; every dWsw and every gradient of the other cases holds on the first term alone,
# worst 8.4e-7 of tau_w = 1e-6 at the single row).  Without the term those dtb elements stand at up to 6.8 tau_w S(|dpre|): where
# sw = 0 every row of a sample has the SAME pre-activation tb[b, h], so one gelu' error adds up over all rows instead of
# averaging.  A_DGELU is at most 4 x the measured figure, the convention of elementwise_check.TAU.
A_MEASURED = 2.35e-8
A_DGELU = 9e-8
TAU_F, TAU_W = TAU[("f32", "fwd")], TAU[("f32", "wgrad")]


def _hidden(M, C):
    return 4 * (M + M * C)


@functools.lru_cache(maxsize=None)
def _operands(B, N, M, C, kind):
    """(sw, wsw, tb, dh0) fp32 on the GPU, made once per case and never written."""
    H = _hidden(M, C)
    rng = np.random.default_rng(1000 * B + N + 7 * M + C)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    logits = rng.standard_normal((B, N, M))
    sw = np.exp(logits) / np.exp(logits).sum(-1, keepdims=True)            # slice weights: a softmax over M
    wsw = rng.standard_normal((H, M)) * (M + M * C) ** -0.5 * 8.0
    tb = rng.standard_normal((B, H)) + 1000.0 * np.arange(B)[:, None]
    dh0 = rng.standard_normal((B, N, H))
    if kind == "sw0":
        sw = np.zeros_like(sw)
    if kind == "scaled":
        wsw = wsw * np.where(np.arange(M) % 2 == 0, 2.0 ** 40, 2.0 ** -40)[None, :]
        tb = tb - 1000.0 * np.arange(B)[:, None]
    return t(sw), t(wsw), t(tb), t(dh0)


@functools.lru_cache(maxsize=None)
def _reference(B, N, M, C, kind):
    """fp64 on the GPU: h0 with its scale, dWsw and dtb with theirs."""
    sw, wsw, tb, dh0 = (x.double() for x in _operands(B, N, M, C, kind))
    pre = (sw @ wsw.t() + tb[:, None, :]).requires_grad_(True)
    h0 = F.gelu(pre)
    (dact,) = torch.autograd.grad(h0.sum(), pre)
    pre_abs = sw.abs() @ wsw.abs().t() + tb.abs()[:, None, :]
    dpre, d_abs = dh0 * dact, dh0.abs()
    flat = lambda x: x.reshape(B * N, -1)
    return dict(h0=h0.detach(), h0_scale=1.13 * pre_abs,
                dw=flat(dpre).t() @ flat(sw), dw_rel=flat(dpre.abs()).t() @ flat(sw).abs(), dw_abs=flat(d_abs).t() @ flat(sw).abs(),
                dtb=dpre.sum(1), dtb_rel=dpre.abs().sum(1), dtb_abs=d_abs.sum(1))


def _check_fwd(got, ref, tag):
    worst = check_products(got, ref["h0"], ref["h0_scale"], TAU_F, rel_ref=R_GELU, label=tag + " h0")
    print(f"{tag}: h0 worst |err| / (1.13 scale) = {worst:.3e} (tau {TAU_F:.1e})")


NEEDED = []          # (label, the absolute coefficient this gradient needs): what A_MEASURED is read from


def _check_grad(got, ref, rel, abs_, label):
    """|got - ref| <= tau_w rel + A_DGELU abs_ per element; prints the worst |err| / rel and the coefficient of abs_ that the
    elements beyond tau_w rel need (the figure A_DGELU is calibrated on) before it asserts."""
    err = (got.double() - ref).abs()
    need = float(((err - TAU_W * rel).clamp_min(0.0) / abs_.clamp_min(1e-300)).max())
    NEEDED.append((label, need))
    print(f"{label}: worst |err| / S(|dpre|) = {float((err / rel.clamp_min(1e-300)).max()):.3e} (tau {TAU_W:.1e}); "
          f"absolute coefficient needed {need:.3e} (A_DGELU {A_DGELU:.1e})")
    check_products(got, ref, rel + (A_DGELU / TAU_W) * abs_, TAU_W, label=label)


def _check_bwd(dw, dtb, ref, tag):
    _check_grad(dw, ref["dw"], ref["dw_rel"], ref["dw_abs"], tag + " dWsw")
    _check_grad(dtb, ref["dtb"], ref["dtb_rel"], ref["dtb_abs"], tag + " dtb")


CASES = [(s, "plain") for s in SHAPES] + [(SHAPES[1], "sw0"), (SHAPES[2], "sw0"), (SHAPES[1], "scaled"), (SHAPES[2], "scaled"),
                                          (SHAPES[3], "scaled")]


@pytest.mark.parametrize("shape,kind", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_entry_kernels_per_element(shape, kind):
    from transformerbasednavierstokesolver_amd import ops
    B, N, M, C = shape
    sw, wsw, tb, dh0 = _operands(B, N, M, C, kind)
    ref = _reference(B, N, M, C, kind)
    tag = f"prev_slice_entry {shape} {kind}"
    h0 = poisoned(ops.prev_slice_entry_fwd, sw, wsw, tb, "gelu")
    _check_fwd(h0, ref, tag)
    if kind == "sw0":          # no product contributes: gelu(tb[b]) in every row, bit for bit
        assert torch.equal(h0, ops.act_fwd(tb, "gelu")[:, None, :].expand(B, N, -1))
    dw, dtb = poisoned(ops.prev_slice_entry_bwd, dh0, sw, wsw, tb, "gelu")
    _check_bwd(dw, dtb, ref, tag)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_fused_equals_three_op_route(shape):
    """functional.prev_slice_entry(fused=False) (row GEMM, broadcast add, activation) meets the same bounds, and so the two
    routes agree within twice them."""
    from transformerbasednavierstokesolver_amd import functional as Fn
    B, N, M, C = shape
    sw, wsw, tb, dh0 = _operands(B, N, M, C, "plain")
    ref = _reference(B, N, M, C, "plain")
    for fused in (True, False):
        w, t = wsw.clone().requires_grad_(True), tb.clone().requires_grad_(True)
        h0 = Fn.prev_slice_entry(sw, w, t, "gelu", fused=fused, engine="f32")
        h0.backward(dh0)
        torch.cuda.synchronize()
        tag = f"prev_slice_entry {shape} {'fused' if fused else 'three-op'}"
        _check_fwd(h0.detach(), ref, tag)
        _check_bwd(w.grad, t.grad, ref, tag)


@pytest.mark.parametrize("shape", SHAPES[:3], ids=lambda v: "x".join(map(str, v)))
def test_autograd_to_the_layer_parameters(shape):
    """tb = Fn.linear(token, Wtok, bias): the gradients of Wsw, Wtok and the bias through functional.prev_slice_entry
    against fp64 autograd of the layer on the explicit concatenation."""
    from transformerbasednavierstokesolver_amd import functional as Fn
    B, N, M, C = shape
    H = _hidden(M, C)
    sw, _, _, dh0 = _operands(B, N, M, C, "plain")
    rng = np.random.default_rng(77 + M)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    weight = t(rng.standard_normal((H, M + M * C)) * (M + M * C) ** -0.5)       # linear_pre's weight, whole
    bias, token = t(rng.standard_normal(H) * 0.1), t(rng.standard_normal((B, 1, M, C)))
    wg, bg = weight.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    tok2 = token.reshape(B, M * C)
    kpad = (-M * C) % 4            # the row GEMM loads 16 bytes at a time along the contraction
    wtok = F.pad(wg[:, M:], (0, kpad)).contiguous()
    tb = Fn.linear(F.pad(tok2, (0, kpad)), wtok, bg, None, engine="f32")
    h0 = Fn.prev_slice_entry(sw, wg[:, :M].contiguous(), tb, "gelu")
    h0.backward(dh0)
    torch.cuda.synchronize()
    # fp64, on the concatenation the kernels never form
    w64, b64 = weight.double().requires_grad_(True), bias.double().requires_grad_(True)
    cat = torch.cat((sw.double(), tok2.double()[:, None, :].expand(B, N, M * C)), -1)
    pre = cat @ w64.t() + b64
    r0 = F.gelu(pre)
    r0.backward(dh0.double())
    p2 = pre.detach().requires_grad_(True)
    (dact,) = torch.autograd.grad(F.gelu(p2).sum(), p2)
    dpre_abs, d_abs = (dh0.double() * dact).abs().reshape(B * N, H), dh0.double().abs().reshape(B * N, H)
    cat_abs = cat.reshape(B * N, -1).abs()
    tag = f"PrevSliceEntryFn {shape}"
    check_products(h0.detach(), r0.detach(), 1.13 * (cat.abs() @ weight.double().abs().t() + bias.double().abs()), TAU_F,
                   rel_ref=R_GELU, label=tag + " h0")
    _check_grad(wg.grad, w64.grad, dpre_abs.t() @ cat_abs, d_abs.t() @ cat_abs, tag + " d linear_pre.weight (Wsw | Wtok)")
    _check_grad(bg.grad, b64.grad, dpre_abs.sum(0), d_abs.sum(0), tag + " d bias")


def test_refusals():
    from transformerbasednavierstokesolver_amd import functional as Fn, ops
    sw, wsw, tb = torch.rand(2, 5, 4, device=DEV), torch.randn(8, 4, device=DEV), torch.randn(2, 8, device=DEV)
    with pytest.raises(ValueError, match="no gradient flows to `sw`"):
        Fn.prev_slice_entry(sw.clone().requires_grad_(True), wsw, tb, "gelu")
    with pytest.raises(ValueError, match="1 <= M <= 64"):
        ops.prev_slice_entry_fwd(torch.rand(1, 2, 65, device=DEV), torch.randn(8, 65, device=DEV), tb[:1], "gelu")
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.prev_slice_entry_fwd(sw, torch.randn(6, 4, device=DEV), torch.randn(2, 6, device=DEV), "gelu")
    with pytest.raises(ValueError, match="262141 row chunks"):        # more units than one launch's grid holds
        ops.prev_slice_entry_fwd(torch.rand(262141, 1, 1, device=DEV), torch.randn(4, 1, device=DEV), torch.randn(262141, 4, device=DEV), "gelu")
    with pytest.raises(TypeError):
        ops.prev_slice_entry_fwd(sw.double(), wsw, tb, "gelu")
    with pytest.raises(ValueError, match="contiguous"):
        ops.prev_slice_entry_fwd(sw, wsw.t().contiguous().t(), tb, "gelu")
