"""Host self-test of the step-tail checks (tests/test_gpu_step_tail_elementwise.py, helpers in elementwise_check.py): no
GPU.  Plain-torch fp32 emulations of the kernels, written in the kernels' own operation order with the coefficient row
rounded once from double (csrc/pa2d_optim.hip: adamw_body, pa2d_adamw_coefficients; pa2d_internal.h: act_bwd, normal_cdf),
stand in for a correct kernel; each corruption changes one thing.  The checks, bounds and inputs are the GPU file's own
(4 x the fp32 CPU yardstick with a floor of 2^-23; parameters N(0, 1) with every third one exactly zero, as biases are).

    corruption                                                         worst |err| / bound   named in the message
    clean emulation, AdamW three steps (n = 5, 1027, 2 097 156)        0.25 (it is the yardstick's arithmetic)
    (a) the scalar tail skipped (n = 1027)                             1.1e+6                3 in the scalar tail
    (b) the tail applied by every workgroup (n = 1027, 2 workgroups)   1.5e+6                3 in the scalar tail
    (c) the second trip skipped (n = 2 097 156)                        7.3e+5                trips [1]
    (d) one float4 stepped twice (n = 1027)                            1.5e+6                trip 0, workgroup 0, thread 77
    (e) bias2 by float powf (the 1e-5 the kernel's comment speaks of)  6.3                   p
    (e') bias1 by float powf, beta1 in {0.85, 0.9, 0.95}               0.44  NOT rejected    -
    (f) 1 - float(beta2) instead of the double                         6.3                   p
    (g) the clip applied although the norm is below max_norm           6.1 in p, and not bit-equal to the unclipped step
    (h) the previous step's beta1                                      8.4e+5                -
    (i) 1 - t*t replaced by 0 beyond |x| > 9                           0.36  NOT rejected    -
    (i') the same beyond |x| > 7                                       13.9                  -
    (j) one probe dropped / doubled in a sum                           exact                 the probe and its trip / tail
    the kernel's activation formulas in fp32 (GELU: the polynomial)    <= 0.51               -

Two limits, recorded rather than hidden:
  * (e') `bias1` by float powf moves lr / bias1 by 2.4e-7 relative at most for beta1 in OneCycle's range (1 - 0.95f against
    0.05): that is the size of one more fp32 rounding, which no fp32 bound can tell from a legitimate operation order.  What
    the kernel's comment calls "off by ~1e-5 at step 1" is bias2 (1 - 0.999f against 1e-3), case (e), which is rejected
    through the parameters that start at zero: there the scale is the update itself.  (f) is caught the same way, in p;
    in v it is 1.3e-8 of the scale v0 + g^2.
  * (i) tanhf(x) rounds to 1 from |x| = 9.02 on, so the clean fp32 `1 - t*t` is 0 or 2^-23 there already, against a true
    value below 6.1e-8: beyond 9 the corruption and the clean kernel differ by less than half an ulp of 1, and the floor of
    the bound (2^-23 absolute on a derivative of magnitude <= 1) is above both.  The check does reject the same corruption
    from |x| > 7 on, where the derivative (3.3e-6) is above the floor.
"""
import math

import numpy as np
import pytest
import torch

import test_gpu_step_tail_elementwise as G
from elementwise_check import (ULP32, adamw_reference, check_abs_rel, decode_probe_sum, exact_sum_probes, flat_where,
                               stream_grid, stream_trips)

BETA2, EPS, WD = G.BETA2, G.EPS, G.WD
f32 = np.float32


# ---------------------------------------------------------------------------------------------- the emulated kernel
def _row(lr, beta1, step, *, bias1_float=False, bias2_float=False, omb2_float=False):
    """pa2d_adamw_coefficients: double arithmetic, each value rounded to float once (or one of the corruptions e, f)."""
    bias1 = float(f32(1) - f32(beta1) ** f32(step)) if bias1_float else 1.0 - beta1 ** step
    bias2 = float(f32(1) - f32(BETA2) ** f32(step)) if bias2_float else 1.0 - BETA2 ** step
    omb2 = float(f32(1) - f32(BETA2)) if omb2_float else 1.0 - BETA2
    return dict(step=f32(lr / bias1), decay=f32(1.0 - lr * WD), omb1=f32(1.0 - beta1), beta2=f32(BETA2), omb2=f32(omb2),
                bias2_sqrt=f32(math.sqrt(bias2)), eps=f32(EPS))


def _body(p, g, m, v, c, coef=1.0):
    """ADAM1 of adamw_body on fp32 tensors (every operation rounds to fp32)."""
    t = lambda x: torch.tensor(x, dtype=torch.float32)
    g_ = g * t(f32(coef))
    p = p * t(c["decay"])
    m = m + t(c["omb1"]) * (g_ - m)
    v = t(c["beta2"]) * v + t(c["omb2"]) * g_ * g_
    p = p - t(c["step"]) * m / (v.sqrt() / t(c["bias2_sqrt"]) + t(c["eps"]))
    return p, m, v


def _emulate(p, g, m, v, c, n, corrupt=None, coef=1.0):
    """One launch over n floats: float4 body in trips of grid * 1024, scalar tail by workgroup 0."""
    n4, grid = 4 * (n // 4), stream_grid(n)
    out = [t.clone() for t in _body(p, g, m, v, c, coef)]
    old = (p, m, v)

    def again(sl):          # the elements of `sl` stepped once more, from the already stepped state
        twice = _body(out[0][sl], g[sl], out[1][sl], out[2][sl], c, coef)
        for o, t in zip(out, twice):
            o[sl] = t

    if corrupt == "tail skipped":
        for o, t in zip(out, old):
            o[n4:] = t[n4:]
    elif corrupt == "tail by every workgroup":
        for _ in range(grid - 1):
            again(slice(n4, n))
    elif corrupt == "second trip skipped":
        for o, t in zip(out, old):
            o[grid * 1024:n4] = t[grid * 1024:n4]
    elif corrupt == "one float4 twice":
        again(slice(4 * 77, 4 * 78))
    else:
        assert corrupt is None, corrupt
    return tuple(out)


def _state(n, kind="normal", seed=0):
    gen = torch.Generator().manual_seed(seed + n)
    p = G._params(n, gen)
    return gen, p, torch.zeros(n), torch.zeros(n)


def _fractions(n, before, after, g, lr, beta1, step, gn64=None, gn32=None, max_norm=0.0, label="emulated"):
    """The GPU file's check of one step (G._check_step's arithmetic) on CPU tensors: the worst fraction of the bound over
    p, m, v; raises like the GPU test does."""
    ref, scale = adamw_reference(*[before[0], g, before[1], before[2]], lr, beta1, BETA2, EPS, WD, step, gn64, max_norm)
    y32, _ = adamw_reference(*[before[0], g, before[1], before[2]], lr, beta1, BETA2, EPS, WD, step, gn32, max_norm,
                             dtype=torch.float32)
    worst = 0.0
    for name, got, r, s, y in zip("pmv", after, ref, scale, y32):
        tau = G._tau(G._yard(y, r, s))
        worst = max(worst, check_abs_rel(got, r, tau * s, 0.0, f"{label} step {step} {name}", n_flat=n))
    return worst


def _rejected(*args, **kw):
    with pytest.raises(AssertionError) as e:
        _fractions(*args, **kw)
    msg = str(e.value)
    ratio = float(msg.split("|err| / bound = ")[1].split(";")[0])
    return ratio, msg


@pytest.mark.parametrize("kind", ["normal", "loguniform"])
@pytest.mark.parametrize("n", [5, 1027, 2097156])
def test_clean_emulation_passes_three_steps(n, kind):
    gen, p, m, v = _state(n, kind)
    worst = 0.0
    for step, (lr, beta1) in enumerate(G.ONE_CYCLE, start=1):
        g = G._grads(kind, n, gen)
        after = _emulate(p, g, m, v, _row(lr, beta1, step), n)
        worst = max(worst, _fractions(n, (p, m, v), after, g, lr, beta1, step))
        p, m, v = after
    print(f"clean emulation n={n} {kind}: worst fraction of the bound {worst:.3f}")
    assert worst <= 0.75, worst          # room between a correct fp32 step and the bound


@pytest.mark.parametrize("corrupt,n,named", [
    ("tail skipped", 1027, "scalar tail"), ("tail by every workgroup", 1027, "scalar tail"),
    ("second trip skipped", 2097156, "trips [1]"), ("one float4 twice", 1027, "trip 0 of 1, workgroup 0 of 2, thread 77")])
def test_structural_corruptions_are_rejected_and_named(corrupt, n, named):
    gen, p, m, v = _state(n)
    (lr, beta1), step = G.ONE_CYCLE[0], 1
    g = G._grads("normal", n, gen)
    after = _emulate(p, g, m, v, _row(lr, beta1, step), n, corrupt)
    ratio, msg = _rejected(n, (p, m, v), after, g, lr, beta1, step)
    print(f"{corrupt}: |err| / bound = {ratio:.3g}\n  {msg}")
    assert ratio > 100 and named in msg, msg
    if "tail" in corrupt:
        assert "0 in the body" in msg and "3 in the scalar tail" in msg, msg


def test_coefficient_corruptions():
    n, step = 4099, 1
    gen, p, m, v = _state(n)
    g = G._grads("normal", n, gen)
    lr, beta1 = G.ONE_CYCLE[0]
    ratios = {}
    for name, kw in (("e bias2 float", dict(bias2_float=True)), ("f omb2 float", dict(omb2_float=True))):
        after = _emulate(p, g, m, v, _row(lr, beta1, step, **kw), n)
        ratios[name], msg = _rejected(n, (p, m, v), after, g, lr, beta1, step)
        assert " p:" in msg, msg          # seen in the parameters that start at zero
    # (e') bias1 by float powf: one more rounding of lr / bias1, below what an fp32 bound can see — recorded, not rejected
    worst = 0.0
    for b1 in (0.85, 0.9, 0.95):
        after = _emulate(p, g, m, v, _row(lr, b1, step, bias1_float=True), n)
        worst = max(worst, _fractions(n, (p, m, v), after, g, lr, b1, step))
        assert abs(float(_row(lr, b1, step, bias1_float=True)["step"]) / (lr / (1 - b1)) - 1) < 3e-7
    ratios["e' bias1 float"] = worst
    # (h) the previous step's beta1
    after = _emulate(p, g, m, v, _row(lr, 0.85, step), n)
    ratios["h stale beta1"], _ = _rejected(n, (p, m, v), after, g, lr, beta1, step)
    print("coefficient corruptions, |err| / bound:", {k: f"{x:.3g}" for k, x in ratios.items()})
    assert ratios["e bias2 float"] > 2 and ratios["f omb2 float"] > 2 and ratios["h stale beta1"] > 100
    assert worst <= 1.0


def test_clip_below_the_norm_is_rejected():
    n, step = 1027, 2
    gen, p, m, v = _state(n)
    g = G._grads("normal", n, gen)
    lr, beta1 = G.ONE_CYCLE[1]
    gn64 = float((g.double() ** 2).sum())
    max_norm = 2.0 * math.sqrt(gn64)
    row = _row(lr, beta1, step)
    plain = _emulate(p, g, m, v, row, n)
    wrong = _emulate(p, g, m, v, row, n, coef=max_norm / (math.sqrt(gn64) + 1e-6))       # q = 2 not limited to 1
    assert not torch.equal(wrong[0], plain[0])                                         # the GPU test's bit comparison
    ratio, _ = _rejected(n, (p, m, v), wrong, g, lr, beta1, step, gn64, float((g ** 2).sum()), max_norm)
    print(f"clip below the norm: |err| / bound = {ratio:.3g} (p, checked first; Adam's update barely depends on the scale of g)")
    assert ratio > 2
    # and the correct clip 10x above passes
    clipped = _emulate(p, g, m, v, row, n, coef=0.1 / (math.sqrt(float((g ** 2).sum())) + 1e-6) * math.sqrt(gn64))
    assert _fractions(n, (p, m, v), clipped, g, lr, beta1, step, gn64, float((g ** 2).sum()), 0.1 * math.sqrt(gn64)) <= 1.0


# ---------------------------------------------------------------------------------------------- sums
def test_probe_sums_decode():
    n = 4195331
    pos = G._probe_positions(n)
    assert pos == [0, 3, 4, 1023, 1024, 2097151, 2097152, 4194304, 4195327, 4195328, 4195329, 4195330]
    assert G._probe_positions(1027) == [0, 3, 4, 1023, 1024, 1025, 1026]
    x = exact_sum_probes(n, pos)
    clean = float((x * x).sum())                       # any order: exact
    assert decode_probe_sum(clean, pos, n) == (True, "exact") and clean == float((x.double() ** 2).sum())
    ok, text = decode_probe_sum(clean - 4.0 ** 6, pos, n)
    assert not ok and "probe 2^6 dropped" in text and "trip 1 of 3, workgroup 0 of 2048, thread 0, component 0" in text, text
    ok, text = decode_probe_sum(clean + 4.0 ** 10, pos, n)
    assert not ok and "probe 2^10 counted twice" in text and "scalar tail, element 1 of 3" in text, text
    ok, text = decode_probe_sum(clean + 4.0 ** 7 - 1.0, pos, n)
    assert not ok and "2^7 counted twice" in text and "2^0 dropped" in text and "trip 2 of 3" in text, text
    assert "not a sum" in decode_probe_sum(float("nan"), pos, n)[1] and "not a sum" in decode_probe_sum(clean + 0.5, pos, n)[1]
    print(text)


def test_flat_where_and_tau_sum():
    assert stream_grid(1) == 1 and stream_grid(1025) == 2 and stream_grid(10 ** 8) == 2048
    assert stream_trips(2097152) == 1 and stream_trips(2097156) == 2 and stream_trips(4195331) == 3 and stream_trips(3) == 0
    assert "scalar tail, element 2 of 3" in flat_where(1026, 1027)
    assert "trip 1 of 2, workgroup 0 of 2048, thread 0, component 3" in flat_where(2097155, 2097156)
    # rel_l2_bwd: 256 workgroups x 256 threads, one float each: four passes up to L = 262 144, a fifth beyond
    assert "body, trip 4 of 5, workgroup 0 of 256, thread 5" in flat_where(262144 + 5, 263171, grid=256, vec=1)
    assert "body, trip 3 of 4, workgroup 255 of 256, thread 255" in flat_where(262143, 262144, grid=256, vec=1)
    assert G.tau_sum(4195331) == pytest.approx(161 * 2.0 ** -24, rel=1e-4) and G.tau_sum(1) == pytest.approx(19 * 2.0 ** -24, rel=1e-4)
    # torch's blocked fp32 sum stands in for the kernel's tree: far inside the derived bound
    for kind in ("normal", "loguniform"):
        g = G._grads(kind, 4195331, torch.Generator().manual_seed(1))
        ref = float((g.double() ** 2).sum())
        assert abs(float((g * g).sum()) - ref) / ref < G.tau_sum(4195331) / 4


def test_check_abs_rel_messages():
    ref = torch.linspace(-2, 2, 4099, dtype=torch.float64)
    got = ref.float().clone()
    assert check_abs_rel(got, ref, ULP32, ULP32, "clean") < 0.6
    assert check_abs_rel(torch.zeros(0), torch.zeros(0), 0.0, 0.0) == 0.0 and check_abs_rel(got * 0, ref * 0, 0.0, 0.0) == 0.0
    got[4096:] += 1e-3
    got[5] = float("nan")
    with pytest.raises(AssertionError) as e:
        check_abs_rel(got, ref, ULP32, ULP32, "corrupt", n_flat=4099)
    msg = str(e.value)
    assert "4 of 4099" in msg and "3 in the scalar tail" in msg and "1 in the body, trips [0]" in msg and "mod 4: [0, 1, 2]" in msg, msg
    assert "index 5 (mod 4 = 1, mod 256 = 5, mod 1024 = 5)" in msg and "thread 1, component 1" in msg, msg


# ---------------------------------------------------------------------------------------------- the trajectory reference
def test_trajectory_reference_and_yardstick():
    init, grads = G._trajectory_inputs()
    h64, h32 = G._torch_adamw(init, grads, torch.float64), G._torch_adamw(init, grads, torch.float32)
    assert len(h64) == G.STEPS + 1 and h64[0].numel() == sum(G.NUMELS)
    stepped = torch.cat([torch.full((k,), i not in G.UNTOUCHED) for i, k in enumerate(G.NUMELS)])
    assert torch.equal(h64[-1][~stepped], h64[0][~stepped]) and int((~stepped).sum()) == 10
    scale = h64[0].abs() + sum((b - a).abs() for a, b in zip(h64[:-1], h64[1:]))
    yard = G._yard(h32[-1][stepped], h64[-1][stepped], scale[stepped])
    print(f"trajectory yardstick {yard:.3e}")
    assert 1e-9 < yard < 1e-6
    # every step clips: the norm of every step's gradients is far above MAX_NORM
    assert all(math.sqrt(sum(float((g ** 2).sum()) for i, g in enumerate(gs) if i not in G.UNTOUCHED)) > 4 * G.MAX_NORM for gs in grads)
    # one parameter off by 1e-5 of its path length is outside the bound
    wrong = h64[-1].clone()
    wrong[6:12] += 1e-5 * scale[6:12]
    with pytest.raises(AssertionError):
        check_abs_rel(wrong[stepped], h64[-1][stepped], G._tau(yard) * scale[stepped], 0.0, "trajectory")


# ---------------------------------------------------------------------------------------------- activations
def _kernel_act(act, x):
    """(act_fwd, act_bwd) of pa2d_internal.h in fp32 torch, operation by operation."""
    one = torch.ones_like(x)
    if act is None:
        return x.clone(), one
    if act == "gelu":          # normal_cdf: Abramowitz-Stegun 7.1.26 on z = |x| / sqrt 2
        z = x.abs() * f32(0.70710678118654752440)
        t = 1.0 / (f32(0.3275911) * z + 1.0)
        poly = f32(1.061405429) * t + f32(-1.453152027)
        for c in (1.421413741, -0.284496736, 0.254829592):
            poly = poly * t + f32(c)
        e = torch.exp(-z * z)
        hq = 0.5 * poly * t * e
        cdf = torch.where(x < 0, hq, 1.0 - hq)
        return x * cdf, x * f32(0.39894228040143267794) * e + cdf
    s = 1.0 / (1.0 + torch.exp(-x))
    if act == "tanh":
        t = torch.tanh(x)
        return t, 1.0 - t * t
    if act == "sigmoid":
        return s, s * (1.0 - s)
    if act == "relu":
        return torch.where(x > 0, x, 0 * x), torch.where(x > 0, one, 0 * one)
    if act == "softplus":
        return torch.where(x > 20, x, torch.log1p(torch.exp(x))), torch.where(x > 20, one, s)
    if act == "ELU":
        return torch.where(x > 0, x, torch.expm1(x)), torch.where(x > 0, one, torch.exp(x))
    assert act == "silu"
    return x / (1.0 + torch.exp(-x)), s * (1.0 + x * (1.0 - s))


def _act_bwd_fraction(act, got, pre, dy):
    yard, tau, _ = G._act_bounds(act, pre, dy)
    _, ref = G._act64(act, pre.double(), dy.double())
    a = dy.double().abs() * (tau + (G.GELU_PHI_ABS if act == "gelu" else 0.0))
    return check_abs_rel(got, ref, a, tau, f"act_bwd {act}", n_flat=pre.numel(), grid=min(8192, -(-pre.numel() // 256)), vec=1)


@pytest.mark.parametrize("act", G.ACTS)
def test_emulated_activations_meet_the_bounds(act):
    """The kernel's own formulas in fp32 meet the act_bwd and epilogue bounds on the grid (GELU: with the polynomial's
    documented error added); this is the derivation of those bounds checked without a GPU."""
    pre = G._act_grid()
    assert pre.numel() == 16384 + 13
    dy = torch.randn(pre.numel(), generator=torch.Generator().manual_seed(11))
    fwd, bwd = _kernel_act(act, pre)
    frac = _act_bwd_fraction(act, dy * bwd, pre, dy)
    ry, rd = G._act64(act, pre.double())
    y32, d32 = G._act64(act, pre)
    fr = []
    for got, ref, r32, extra in ((fwd, ry, y32, G.GELU_PHI_ABS * pre.double().abs()), (bwd, rd, d32, G.GELU_PHI_ABS)):
        tau = G._tau(G._yard(r32, ref, 1.0 + ref.abs()))
        fr.append(check_abs_rel(got, ref, tau + (extra if act == "gelu" else 0.0), tau, f"epilogue {act}"))
    print(f"emulated {act}: act_bwd {frac:.3f}, epilogue y {fr[0]:.3f}, act' {fr[1]:.3f} of their bounds")
    assert max(frac, *fr) <= 1.0


def test_tanh_derivative_zeroed_in_the_tail():
    pre = G._act_grid()
    dy = torch.ones(pre.numel())
    _, clean = _kernel_act("tanh", pre)
    fractions = {}
    for cut in (9.0, 7.0):
        got = torch.where(pre.abs() > cut, torch.zeros_like(clean), clean)
        if cut == 9.0:          # indistinguishable from the clean fp32 formula: see the module docstring
            assert float((got - clean).abs().max()) <= ULP32
            fractions[cut] = _act_bwd_fraction("tanh", got, pre, dy)
        else:
            with pytest.raises(AssertionError) as e:
                _act_bwd_fraction("tanh", got, pre, dy)
            fractions[cut] = float(str(e.value).split("|err| / bound = ")[1].split(";")[0])
    print("tanh' zeroed beyond |x| > cut, |err| / bound:", fractions)
    assert fractions[9.0] <= 1.0 < fractions[7.0]
