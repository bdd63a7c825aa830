"""The kernels that end every training iteration, element by element against fp64: the clip norm (pa2d_sumsq and its
second pass pa2d_launch_reduce), AdamW (pa2d_adamw_step / pa2d_adamw_step_dev, and FusedAdamW over several active
ranges), the relative L2 loss (pa2d_rel_l2_fwd / pa2d_rel_l2_bwd), pa2d_act_bwd and the act_fwd / act_bwd tails of the GEMM
epilogues.  Every reference is plain fp64 torch on the device, computed from the fp32 values the kernel was given.
Everything a kernel reads or updates in place sits between guard bands (`_banded`), asserted after every launch;
everything an op allocates goes through `poisoned`.

Kernel coverage:

    sumsq_partial_kernel + reduce_slabs_kernel   n = 0, 1 .. 4 195 331: one workgroup, the 2048-workgroup cap, one float4 into
                                                 the second trip, two trips and a partial third with a 3-element tail
    adamw_kernel / adamw_dev_kernel              the same sizes, three consecutive steps, clip on / off / not biting
    FusedAdamW.step / stage_step + step_staged   three active ranges with padded slots, 12 OneCycle steps
    rel_l2_fwd_kernel / rel_l2_bwd_kernel        L = 1 .. 263 171 (the backward's grid is capped at 256 x 256 threads of one float:
                                                 four passes up to L = 262 144, a fifth beyond)
    act_bwd_kernel                               all eight activations; n = 1, the grid, 8192 * 256 + 3 (second trip)
    GEMM epilogues (act_fwd, saved derivative)   gemm_kc_kernel (f32), the small split kernel, gemm_rowpanel_kernel
    LinearFn                                     act_bwd + weight / data gradients, M = 333, K = 76, N = 128, silu
  Not tested: pa2d_rel_l2_bwd puts B on gridDim.y (limit 65 535); no case comes near it.

Exact probes.  A gradient that is zero except for 2^j at <= 12 positions has squares 4^j; every subset sum (and every sum
with one probe counted twice) is below 2^24, so the result must equal sum 4^j bit for bit in any order, and the base-4
digits of a wrong result say which probe was dropped or doubled (elementwise_check.decode_probe_sum).

Derived bounds (u = 2^-24, one fp32 rounding; all terms of these sums are >= 0, so a value that passes through D roundings
is off by at most D u (1 + D u) relative):

  tau_sum(n) = D(n) u.  sumsq_partial_kernel: per trip a thread squares four values and adds them to its sum, at most 5
  roundings on the path of any term (product, three adds, the add into s; FMA contraction only removes some), T =
  ceil((n / 4) / (grid * 256)) trips, 2 more for a scalar-tail element (workgroup 0), 6 for the 64-lane butterfly, 2 for
  (red0 + red1) + (red2 + red3).  reduce_slabs_kernel over `grid` partials: each of 4 lanes walks c = ceil(grid / 4)
  partials over four accumulators, ceil(c / 4) + 3 adds on the longest (the remainder loop feeds s0), 2 for (s0 + s1) +
  (s2 + s3), 3 for the four lanes.  D = 5 T + 2 [n % 4 > 0] + 8 + ceil(ceil(grid / 4) / 4) + 8: 161 at n = 4 195 331
  (9.6e-6), 19 at n = 1 (1.1e-6).
  rel_l2_fwd_kernel: T = ceil(L / 256) adds per thread, 1 for the product, 6 + 2 for the block sum: D_y = T + 9; the
  difference pred - y is rounded once before it is squared (2 more): D_d = T + 11.  The roots halve the relative error and
  round once: tau_yn = (D_y / 2 + 1) u, tau_dn = (D_d / 2 + 1) u, and the quotient tau_ratio = tau_dn + tau_yn + u.
  GELU: pa2d_internal.h evaluates erfc by Abramowitz-Stegun 7.1.26, |eps| <= 1.5e-7, so Phi(x) = 1 - erfc / 2 (or
  erfc / 2) is off by <= 7.5e-8 absolute: x Phi(x) by 7.5e-8 |x|, and Phi(x) + x phi(x) by 7.5e-8 (the density term has no
  polynomial).  These are added to the yardstick bound of the GELU cases.

Yardstick bounds.  Everywhere else the bound is 4 x the worst error of the same fp64 statement evaluated by torch in fp32
on the CPU, on the test's own inputs, with a floor of one ulp (2^-23): per element |got - ref| <= tau * scale with the scales
of elementwise_check.adamw_reference for p, m, v; tau |ref| for the loss gradient; tau |dy| (1 + |act'|) for act_bwd and
tau (1 + |ref|) for the epilogues (a = r = tau in |got - ref| <= a + r |ref|).  The FusedAdamW trajectory is measured against
fp64 torch.optim.AdamW + clip_grad_norm_ with scale |p0| + sum_t |p_t - p_(t-1)|, yardstick fp32 torch.optim.AdamW.

Kinks.  relu'(+-0) = 0 and ELU'(+-0) = 1: what torch's fp32 backward returns (relu: grad * (y > 0); elu: the x <= 0
branch, exp(0)); softplus switches to the identity at x > 20 exactly as F.softplus's threshold does.

CALIBRATION (one MI355X; worst |err| / scale of the fp32 CPU yardstick, the bound = max(4 x yardstick, 2^-23) or the derived
bound, and the kernel's measured worst, each at the case where measured / bound is largest; the module prints this table
under pytest -s):

    op / case family                   yardstick   bound      measured   case
    sumsq exact probes                 -           0 (bits)   0          n = 1027 (7 probes), 4 195 331 (12 probes)
    sumsq random N(0, 1)               -           1.43e-6    6.74e-8    n = 1025 (tau_sum: 24 u); 9.6e-6 at n = 4 195 331
    sumsq random log-uniform           -           1.13e-6    6.35e-8    n = 3 (tau_sum: 19 u)
    adamw_step, adamw_step_dev  p      2.57e-8     1.19e-7    4.08e-8    N(0, 1) n = 1 step 2 (the two forms: the same figures)
                                m      3.65e-8     1.46e-7    4.01e-8    N(0, 1) n = 1027 step 2
                                v      4.70e-8     1.88e-7    4.70e-8    log-uniform n = 3 step 2
    adamw clip (a), (d)         p      1.94e-7     7.77e-7    1.97e-7    (a) n = 1027
                                m      4.45e-8     1.78e-7    4.68e-8    (a) n = 1027
                                v      5.38e-8     2.15e-7    5.38e-8    (a) n = 3
    adamw clip (b), (c)                -           0 (bits)   0          equal to the unclipped step
    FusedAdamW 12-step trajectory      4.90e-7     1.96e-6    3.34e-7    numels [1, 5, 1023, 4, 7, 1025, 3, 2]
    rel_l2_fwd probes dn, yn / ratio   -           1 / 2 ulp  0 / 0      all seven (B, L)
    rel_l2_fwd random dn               -           4.17e-7    7.92e-8    B = 2 L = 255 (derived; 3.1e-5 at L = 263 171)
                      yn               -           3.58e-7    5.89e-8    B = 2 L = 255
                      ratio            -           8.35e-7    1.10e-7    B = 2 L = 255
    rel_l2_bwd                         4.77e-8     1.91e-7    4.77e-8    B = 1 L = 1
    act_bwd      gelu (+ 7.5e-8 |dy|)  9.75e-10    1.19e-7    9.42e-8    n = 1
                 tanh                  5.99e-8     2.40e-7    7.53e-8    second trip
                 sigmoid               8.79e-8     3.52e-7    8.79e-8    grid
                 softplus              8.34e-8     3.34e-7    7.27e-8    second trip
                 ELU                   4.86e-8     1.94e-7    4.45e-8    second trip
                 silu                  4.93e-7     1.97e-6    4.93e-7    grid (s (1 + x (1 - s)) loses 1 - s near x = 15, in torch too)
                 relu, None            0           1.19e-7    0
    epilogue y / act'  gelu            8.80e-8 / 5.39e-8   3.52e-7 / 2.16e-7 (+ 7.5e-8 |x| / 7.5e-8)   1.29e-7 / 1.03e-7
                       tanh            1.88e-8 / 5.99e-8   1.19e-7 / 2.40e-7   3.42e-8 / 6.40e-8
                       sigmoid         4.40e-8 / 8.79e-8   1.76e-7 / 3.51e-7   4.40e-8 / 8.79e-8
                       softplus        5.61e-8 / 4.25e-8   2.25e-7 / 1.70e-7   5.30e-8 / 4.40e-8
                       ELU             2.98e-8 / 2.42e-8   1.19e-7 / 1.19e-7   2.12e-8 / 1.99e-8
                       silu            9.64e-8 / 4.86e-7   3.86e-7 / 1.95e-6   9.64e-8 / 4.86e-7
                       relu            0 / 0               1.19e-7             0 / 0
                       (M = 257, K = N = 64, f32; the split engine and the row-stationary kernel give the same figures)
    LinearFn y, dx / dw, db            -           1.6e-6 / 1e-6 (TAU)   1.9e-7 / 7.3e-8   split; f32: 1.7e-7 / 7.3e-8

No kernel exceeds a bound and none had to change.  Where measured equals the yardstick (sigmoid, silu, v, the loss gradient)
the kernel evaluates the same expression as torch's fp32 kernels.  The corruptions these bounds reject, and the two they
cannot (a float `bias1`, and `1 - t*t` zeroed beyond |x| > 9, both below one fp32 rounding), are emulated on the host in
test_step_tail_host.py.
"""
import math

import numpy as np
import pytest
import torch

from elementwise_check import (EPS32, TAU, ULP32, adamw_reference, check_abs_rel, check_products, decode_probe_sum,
                               exact_sum_probes, flat_where, poisoned, stream_grid, stream_trips)
from test_gpu_graphed_steps import _banded, _bands_untouched

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BETA2, EPS, WD = 0.999, 1e-8, 1e-2
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 1027, 2097152, 2097156, 4195331]
TRIP = 2048 * 1024                     # floats of one full trip of the capped grid
GELU_PHI_ABS = 0.5 * 1.5e-7            # |Phi_kernel - Phi| from the erfc polynomial's documented 1.5e-7

WORST = {}      # family -> [(measured, bound, yardstick or None, case), ...]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nstep tail: worst measured |err| / scale per family (measured, bound, yardstick):")
    for k in sorted(WORST):
        v, bound, yard, case = max(WORST[k], key=lambda t: t[0] / t[1] if t[1] else t[0])
        print(f"  {k:34s} measured {v:.3e}  bound {bound:.3e}  yardstick {'-' if yard is None else f'{yard:.3e}'}   {case}")


def _note(fam, measured, bound, yard, case):
    WORST.setdefault(fam, []).append((measured, bound, yard, case))


def _yard(got32, ref64, scale):
    """Worst |fp32 statement - fp64 statement| / scale: the yardstick."""
    err = (got32.double() - ref64).abs()
    ok = scale > 0
    return float((err[ok] / scale[ok]).max()) if bool(ok.any()) else 0.0


def _tau(yard):
    return max(4.0 * yard, ULP32)


def _grads(kind, n, gen):
    """N(0, 1), or a log-uniform magnitude over [2^-30, 2^10] with a random sign (eps matters for some elements only)."""
    if kind == "normal":
        return torch.randn(n, generator=gen)
    mag = torch.exp2(torch.rand(n, generator=gen, dtype=torch.float64) * 40.0 - 30.0)
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    return (mag * sign).float()


def _params(n, gen):
    """N(0, 1) with every third parameter exactly zero, as biases start: there the scale of p is the update itself, so an
    error in the step size is not hidden behind |p|."""
    p = torch.randn(n, generator=gen)
    p[1::3] = 0.0
    return p


# ---------------------------------------------------------------------------------------------- sumsq
def tau_sum(n):
    grid = stream_grid(n)
    per_lane = -(-grid // 4)                    # partials one lane of reduce_slabs_kernel walks
    d = 5 * stream_trips(n) + (2 if n % 4 else 0) + 8 + -(-per_lane // 4) + 8
    return d * EPS32 * (1.0 + d * EPS32)


def _probe_positions(n):
    """Elements 0, 3, 4, 1023, 1024; the last of the first trip and the first of the second; the first of the third; the
    last float4 element; each tail element — those that exist at this n."""
    n4 = 4 * (n // 4)
    want = [0, 3, 4, 1023, 1024, TRIP - 1, TRIP, 2 * TRIP, n4 - 1] + list(range(n4, n))
    out = []
    for q in want:
        if 0 <= q < n and q not in out:
            out.append(q)
    return out


def _sumsq(g):
    from transformerbasednavierstokesolver_amd import ops
    buf, view = _banded(g.to(DEV))
    out = poisoned(ops.sumsq, view)
    assert _bands_untouched(buf, g.numel()) and torch.equal(view, g.to(DEV))
    return out


@pytest.mark.parametrize("n", [1027, 4195331])
def test_sumsq_exact_probes(n):
    pos = _probe_positions(n)
    assert len(pos) == (12 if n > 2 * TRIP else 7)
    got = _sumsq(exact_sum_probes(n, pos))
    ok, text = decode_probe_sum(float(got), pos, n)
    print(f"sumsq probes n={n}: {text}")
    assert ok, f"sumsq n={n}: {text}"
    # one probe at a time as well: a dropped and a doubled element cannot cancel
    for j, q in enumerate(pos):
        x = torch.zeros(n)
        x[q] = 2.0 ** j
        one = float(_sumsq(x))
        assert one == 4.0 ** j, f"sumsq n={n}: a single probe 2^{j}: got {one}, want {4.0 ** j}, at {flat_where(q, n)}"
    _note("sumsq exact probes", 0.0, 0.0, None, f"n={n}")


def test_sumsq_of_nothing_is_zero_and_a_misaligned_view_is_refused():
    from transformerbasednavierstokesolver_amd import ops
    out = poisoned(ops.sumsq, torch.empty(0, device=DEV))
    assert out.shape == (1,) and float(out) == 0.0
    buf = torch.ones(16, device=DEV)
    with pytest.raises(RuntimeError, match="PA2D_ERR_ARG"):
        ops.sumsq(buf[1:9])
    torch.cuda.synchronize()
    assert float(ops.sumsq(buf[4:12])) == 8.0


@pytest.mark.parametrize("kind", ["normal", "loguniform"])
@pytest.mark.parametrize("n", SIZES)
def test_sumsq_random(n, kind):
    g = _grads(kind, n, torch.Generator().manual_seed(7 * n + len(kind)))
    got = float(_sumsq(g))
    ref = float((g.to(DEV).double() ** 2).sum())
    rel = abs(got - ref) / ref
    bound = tau_sum(n)
    print(f"sumsq {kind} n={n}: |got - ref| / ref = {rel:.3e}, tau_sum = {bound:.3e}")
    _note(f"sumsq random {kind}", rel, bound, None, f"n={n}")
    assert rel <= bound, (f"sumsq {kind} n={n}: got {got!r}, fp64 {ref!r}: got / ref - 1 = {got / ref - 1:+.3e} exceeds tau_sum = "
                          f"{bound:.3e} ({'too large: elements counted twice' if got > ref else 'too small: elements dropped'}; "
                          f"{stream_grid(n)} workgroups, {stream_trips(n)} trips of the float4 body, {n % 4} tail elements)")


# ---------------------------------------------------------------------------------------------- AdamW, one step at a time
ONE_CYCLE = [(1e-3, 0.95), (1e-2, 0.85), (1e-3, 0.9)]          # (lr, beta1) of three consecutive steps


def _launch(form, p, g, m, v, lr, beta1, step, gn=None, max_norm=0.0):
    from transformerbasednavierstokesolver_amd import ops
    if form == "arg":
        ops.adamw_step(p, g, m, v, lr, beta1, BETA2, EPS, WD, step, gn, max_norm)
    else:
        row = ops.adamw_coefficients(lr, beta1, BETA2, EPS, WD, step, max_norm).to(DEV)
        ops.adamw_step_dev(p, g, m, v, row, gn)
    torch.cuda.synchronize()


def _check_step(fam, label, n, state, g, lr, beta1, step, gnorm_sq64=None, gnorm_sq32=None, max_norm=0.0):
    """`state`: the kernel's (p, m, v) before and after the launch.  Bounds every element of p, m, v against the fp64
    statement applied to the state before; the yardstick is the fp32 statement on the CPU."""
    (p0, m0, v0), after = state
    ref, scale = adamw_reference(p0, g, m0, v0, lr, beta1, BETA2, EPS, WD, step, gnorm_sq64, max_norm)
    cpu = [t.cpu() for t in (p0, g, m0, v0)]
    ref_c, scale_c = adamw_reference(*cpu, lr, beta1, BETA2, EPS, WD, step, gnorm_sq64, max_norm)
    y32, _ = adamw_reference(*cpu, lr, beta1, BETA2, EPS, WD, step, gnorm_sq32, max_norm, dtype=torch.float32)
    for name, got, r, s, rc, sc, y in zip("pmv", after, ref, scale, ref_c, scale_c, y32):
        yard = _yard(y, rc, sc)
        tau = _tau(yard)
        frac = check_abs_rel(got, r, tau * s, 0.0, f"{label} step {step} {name}", n_flat=n)
        print(f"{label} step {step} {name}: measured {frac * tau:.3e}, bound {tau:.3e}, yardstick {yard:.3e}")
        _note(f"{fam} {name}", frac * tau, tau, yard, f"{label} step {step}")


@pytest.mark.parametrize("kind", ["normal", "loguniform"])
@pytest.mark.parametrize("form", ["arg", "dev"])
@pytest.mark.parametrize("n", SIZES)
def test_adamw_three_steps_elementwise(n, form, kind):
    gen = torch.Generator().manual_seed(1000 + 3 * n + len(kind))
    bufs = [_banded(t) for t in (_params(n, gen).to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV))]
    (_, p), (_, m), (_, v) = bufs
    for step, (lr, beta1) in enumerate(ONE_CYCLE, start=1):
        g0 = _grads(kind, n, gen).to(DEV)
        gbuf, g = _banded(g0)
        before = tuple(t.clone() for t in (p, m, v))
        _launch(form, p, g, m, v, lr, beta1, step)
        assert _bands_untouched(gbuf, n) and torch.equal(g, g0), "the gradient is read only"
        assert all(_bands_untouched(b, n) for b, _ in bufs), (form, n, step)
        _check_step(f"adamw_step{'_dev' if form == 'dev' else ''}", f"adamw {form} {kind} n={n}", n,
                    (before, (p, m, v)), g, lr, beta1, step)
        assert not torch.equal(p, before[0])


@pytest.mark.parametrize("form", ["arg", "dev"])
@pytest.mark.parametrize("n", [3, 1027, 2097156])
def test_adamw_clip_cases(n, form):
    from transformerbasednavierstokesolver_amd import ops
    gen = torch.Generator().manual_seed(77 + n)
    p0, g0 = _params(n, gen).to(DEV), torch.randn(n, generator=gen).to(DEV)
    m0, v0 = 0.1 * torch.randn(n, generator=gen).to(DEV), 0.1 * torch.rand(n, generator=gen).to(DEV)
    gbuf, g = _banded(g0)
    gn = ops.sumsq(g)
    gn64 = float((g0.double() ** 2).sum())
    norm = math.sqrt(gn64)
    lr, beta1, step = 1e-2, 0.9, 3

    def run(g_view, gnorm, max_norm, start=(p0, m0, v0)):
        bufs = [_banded(t) for t in start]
        _launch(form, bufs[0][1], g_view, bufs[1][1], bufs[2][1], lr, beta1, step, gnorm, max_norm)
        assert all(_bands_untouched(b, n) for b, _ in bufs) and _bands_untouched(gbuf, n)
        return tuple(t for _, t in bufs)

    plain = run(g, None, 0.0)
    # (a) the norm is 10x above max_norm: the reference clips with the fp64 norm, the yardstick with the fp32 sum
    a = run(g, gn, norm / 10.0)
    _check_step("adamw clip", f"adamw {form} clip (a) n={n}", n, ((p0, m0, v0), a), g, lr, beta1, step, gn64,
                float((g0.cpu() ** 2).sum()), norm / 10.0)
    assert not torch.equal(a[1], plain[1])
    # (b) the norm is below max_norm, (c) max_norm = 0 with the norm given: the unclipped step, bit for bit
    for tag, max_norm in (("b", 2.0 * norm), ("c", 0.0)):
        got = run(g, gn, max_norm)
        assert all(torch.equal(x, y) for x, y in zip(got, plain)), f"clip case ({tag}) n={n} differs from the unclipped step"
    # (d) an all-zero gradient with clipping on: p only decays, m and v stay 0, everything finite
    zbuf, z = _banded(torch.zeros(n, device=DEV))
    zeros = torch.zeros(n, device=DEV)
    d = run(z, ops.sumsq(z), 0.1, start=(p0, zeros, zeros))
    assert _bands_untouched(zbuf, n) and all(bool(torch.isfinite(t).all()) for t in d)
    assert float(d[1].abs().max()) == 0.0 == float(d[2].abs().max())
    assert torch.equal(d[0], p0 * torch.tensor(1.0 - lr * WD, dtype=torch.float32, device=DEV)), "p must only decay"
    _check_step("adamw clip", f"adamw {form} clip (d) n={n}", n, ((p0, zeros, zeros), d), z, lr, beta1, step, 0.0, 0.0, 0.1)


@pytest.mark.parametrize("form", ["arg", "dev"])
def test_adamw_refuses_a_misaligned_buffer_and_writes_nothing(form):
    n = 8
    for which in range(4):          # p, g, m, v in turn as an offset-1 view
        whole = [torch.full((n + 4,), 0.5, device=DEV) for _ in range(4)]
        views = [t[1:n + 1] if i == which else t[4:] for i, t in enumerate(whole)]
        with pytest.raises(RuntimeError, match="PA2D_ERR_ARG"):
            _launch(form, views[0], views[1], views[2], views[3], 1e-3, 0.9, 1)
        torch.cuda.synchronize()
        assert all(bool((t == 0.5).all()) for t in whole), ("pgmv"[which], form)


# ---------------------------------------------------------------------------------------------- FusedAdamW, several ranges
NUMELS = [1, 5, 1023, 4, 7, 1025, 3, 2]
UNTOUCHED = (4, 6)                    # the parameters of 7 and 3 elements never receive a gradient
STEPS, MAX_NORM, MAX_LR = 12, 0.5, 1e-2


def _trajectory_inputs():
    gen = torch.Generator().manual_seed(2024)
    init = [torch.randn(k, generator=gen) for k in NUMELS]
    grads = [[torch.randn(k, generator=gen) * (0.2 + 0.3 * t) for k in NUMELS] for t in range(STEPS)]
    return init, grads


def _torch_adamw(init, grads, dtype):
    """torch.optim.AdamW + clip_grad_norm_ + OneCycleLR on CPU copies in `dtype`: the parameters after every step."""
    ps = [torch.nn.Parameter(t.to(dtype).clone()) for t in init]
    opt = torch.optim.AdamW(ps, lr=MAX_LR, betas=(0.9, BETA2), eps=EPS, weight_decay=WD)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=MAX_LR, total_steps=STEPS)
    hist = [torch.cat([p.detach().clone() for p in ps])]
    for t in range(STEPS):
        for i, p in enumerate(ps):
            p.grad = None if i in UNTOUCHED else grads[t][i].to(dtype).clone()
        torch.nn.utils.clip_grad_norm_(ps, MAX_NORM)
        opt.step()
        sched.step()
        hist.append(torch.cat([p.detach().clone() for p in ps]))
    return hist


def _fused(init, grads, staged):
    from transformerbasednavierstokesolver_amd.optim import FusedAdamW
    ps = [torch.nn.Parameter(t.to(DEV).clone()) for t in init]
    opt = FusedAdamW(ps, lr=MAX_LR, betas=(0.9, BETA2), eps=EPS, weight_decay=WD, max_grad_norm=MAX_NORM)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=MAX_LR, total_steps=STEPS)
    for t in range(STEPS):
        opt.zero_grad()
        # autograd hands every stepped parameter exactly grads[t][i] (the bucket's views are zero before)
        sum((p * grads[t][i].to(DEV)).sum() for i, p in enumerate(ps) if i not in UNTOUCHED).backward()
        if staged:
            opt.stage_step()
            opt.step_staged()
        else:
            opt.step()
        sched.step()
    torch.cuda.synchronize()
    return ps, opt


def test_fused_adamw_several_active_ranges():
    init, grads = _trajectory_inputs()
    ps, opt = _fused(init, grads, staged=False)
    sync = opt.sync
    assert sync.active_ranges() == [(0, 1040), (1048, 2076), (2080, 2084)] and sync.total == 2084
    h64, h32 = _torch_adamw(init, grads, torch.float64), _torch_adamw(init, grads, torch.float32)
    scale = h64[0].abs() + sum((b - a).abs() for a, b in zip(h64[:-1], h64[1:]))
    stepped = torch.cat([torch.full((k,), i not in UNTOUCHED) for i, k in enumerate(NUMELS)])
    yard = _yard(h32[-1][stepped], h64[-1][stepped], scale[stepped])
    tau = _tau(yard)
    got = torch.cat([p.detach().reshape(-1) for p in ps]).cpu()
    assert not torch.equal(got[stepped], h64[0][stepped].float())
    frac = check_abs_rel(got[stepped], h64[-1][stepped], tau * scale[stepped], 0.0, "FusedAdamW 12 steps, stepped elements")
    print(f"FusedAdamW trajectory: measured {frac * tau:.3e}, bound {tau:.3e}, yardstick {yard:.3e}")
    _note("FusedAdamW 12-step trajectory", frac * tau, tau, yard, f"numels {NUMELS}")
    # the two parameters without a gradient: bit-unchanged, .grad is None, moments exactly 0
    pad = torch.ones(sync.total, dtype=torch.bool)
    for i, (p, off) in enumerate(zip(ps, sync.offsets)):
        pad[off:off + NUMELS[i]] = False
        if i in UNTOUCHED:
            assert torch.equal(p.detach().cpu(), init[i]) and p.grad is None, i
            for buf in (opt.exp_avg, opt.exp_avg_sq):
                assert float(buf[off:off + NUMELS[i]].abs().max()) == 0.0, i
        else:
            assert p.grad is not None and float(opt.exp_avg_sq[off:off + NUMELS[i]].min()) > 0.0, i
    # every padding element of all four flat buffers is exactly 0
    assert int(pad.sum()) == 2084 - sum(NUMELS)
    for name, buf in (("p", opt.flat_p), ("g", sync.flat), ("m", opt.exp_avg), ("v", opt.exp_avg_sq)):
        assert float(buf[pad.to(DEV)].abs().max()) == 0.0, f"padding of flat {name} was written"
    # the twin driven by stage_step() + step_staged(): the same bits
    ps2, opt2 = _fused(init, grads, staged=True)
    for name, a, b in (("p", opt.flat_p, opt2.flat_p), ("m", opt.exp_avg, opt2.exp_avg), ("v", opt.exp_avg_sq, opt2.exp_avg_sq)):
        assert torch.equal(a, b), f"staged twin differs in flat {name} at {(a != b).nonzero().flatten()[:8].tolist()}"
    assert opt2.steps == opt.steps == STEPS


# ---------------------------------------------------------------------------------------------- relative L2
REL_CASES = [(1, 1), (3, 3), (2, 255), (2, 256), (3, 257), (5, 4099), (2, 262144 + 1024 + 3)]
GOUT = [1.3, -0.7, 0.0, 0.25, -2.0]


def _banded2d(t):
    buf, view = _banded(t.reshape(-1).to(DEV))
    return buf, view.view(t.shape)


def _ulps(a, b):
    """Distance in fp32 ulps between positive fp32 tensors."""
    return (a.contiguous().view(torch.int32).long() - b.contiguous().view(torch.int32).long()).abs()


@pytest.mark.parametrize("B,L", REL_CASES)
def test_rel_l2_forward_exact_probes(B, L):
    from transformerbasednavierstokesolver_amd import ops
    pos = [q for q in dict.fromkeys([0, 255, 256, L - 1]) if 0 <= q < L]
    y, pred = torch.zeros(B, L), torch.zeros(B, L)
    for b in range(B):
        for j, q in enumerate(pos):
            y[b, q] = 2.0 ** (j + b)              # y^2 = 4^(j + b); pred - y = 2^(j + b + 1), squares 4^(j + b + 1)
            pred[b, q] = 3.0 * 2.0 ** (j + b)
    (pb, p), (yb, yv) = _banded2d(pred), _banded2d(y)
    dn, yn, ratio = poisoned(ops.rel_l2_fwd, p, yv)
    assert _bands_untouched(pb, B * L) and _bands_untouched(yb, B * L)
    sy = torch.tensor([sum(4.0 ** (j + b) for j in range(len(pos))) for b in range(B)], dtype=torch.float64)
    want_yn, want_dn = sy.sqrt().float(), (4.0 * sy).sqrt().float()
    for b in range(B):
        seen_y, seen_d = float(yn[b]) ** 2 / 4.0 ** b, float(dn[b]) ** 2 / 4.0 ** (b + 1)
        text = (f"rel_l2_fwd B={B} L={L} sample {b}: ynorm^2 reads as {decode_probe_sum(round(seen_y), pos)[1]}; "
                f"dnorm^2 as {decode_probe_sum(round(seen_d), pos)[1]} (probe positions {pos})")
        assert int(_ulps(yn[b:b + 1].cpu(), want_yn[b:b + 1])) <= 1 and int(_ulps(dn[b:b + 1].cpu(), want_dn[b:b + 1])) <= 1, text
        assert int(_ulps(ratio[b:b + 1].cpu(), torch.tensor([2.0]))) <= 2, text
    worst = max(int(_ulps(yn.cpu(), want_yn).max()), int(_ulps(dn.cpu(), want_dn).max()))
    _note("rel_l2_fwd probes (ulp)", float(max(worst, int(_ulps(ratio.cpu(), torch.full((B,), 2.0)).max()))), 2.0, None,
          f"B={B} L={L}")


@pytest.mark.parametrize("B,L", REL_CASES)
def test_rel_l2_forward_and_backward_random(B, L):
    from transformerbasednavierstokesolver_amd import ops
    gen = torch.Generator().manual_seed(31 * B + L)
    y = torch.randn(B, L, generator=gen)
    pred = y + 0.3 * torch.randn(B, L, generator=gen)
    (pb, p), (yb, yv) = _banded2d(pred), _banded2d(y)
    dn, yn, ratio = poisoned(ops.rel_l2_fwd, p, yv)
    d64, y64 = (p.double() - yv.double()), yv.double()
    rdn, ryn = d64.norm(dim=1), y64.norm(dim=1)
    T = -(-L // 256)
    tau_yn, tau_dn = ((T + 9) / 2 + 1) * EPS32, ((T + 11) / 2 + 1) * EPS32
    for name, got, ref, tau in (("dn", dn, rdn, tau_dn), ("yn", yn, ryn, tau_yn), ("ratio", ratio, rdn / ryn, tau_dn + tau_yn + EPS32)):
        frac = check_abs_rel(got, ref, 0.0, tau * (1 + tau), f"rel_l2_fwd B={B} L={L} {name}")
        print(f"rel_l2_fwd B={B} L={L} {name}: measured {frac * tau:.3e}, derived bound {tau:.3e}")
        _note(f"rel_l2_fwd random {name}", frac * tau, tau, None, f"B={B} L={L}")
    # backward: per-sample gout of mixed sign and one zero; reference from the fp32 dn, yn the kernel is given
    gout = torch.tensor(GOUT[:B], device=DEV)
    dpred = poisoned(ops.rel_l2_bwd, p, yv, dn, yn, gout)
    assert _bands_untouched(pb, B * L) and _bands_untouched(yb, B * L)
    ref = (gout.double() / (dn.double() * yn.double()))[:, None] * d64
    pc, yc, dnc, ync, gc = (t.cpu() for t in (p, yv, dn, yn, gout))
    y32 = (gc / (dnc * ync))[:, None] * (pc - yc)
    yard = _yard(y32, ref.cpu(), ref.cpu().abs())
    tau = _tau(yard)
    for b in range(B):          # per sample, so that the message's trip / index is the position inside the sample
        frac = check_abs_rel(dpred[b], ref[b], 0.0, tau, f"rel_l2_bwd B={B} L={L} sample {b}", n_flat=L,
                             grid=min(256, -(-L // 1024)), vec=1)
        _note("rel_l2_bwd", frac * tau, tau, yard, f"B={B} L={L}")
    if B >= 3:
        assert float(dpred[2].abs().max()) == 0.0          # gout = 0


def test_rel_l2_backward_no_samples_and_a_zero_difference():
    from transformerbasednavierstokesolver_amd import ops
    e = torch.empty(0, 7, device=DEV)
    z = torch.empty(0, device=DEV)
    assert ops.rel_l2_bwd(e, e, z, z, z).shape == (0, 7)
    torch.cuda.synchronize()
    y = torch.randn(2, 300, generator=torch.Generator().manual_seed(5)).to(DEV)
    dn, yn, ratio = poisoned(ops.rel_l2_fwd, y.clone(), y)
    assert float(dn.abs().max()) == 0.0 == float(ratio.abs().max())
    d = poisoned(ops.rel_l2_bwd, y.clone(), y, dn, yn, torch.ones(2, device=DEV))
    assert float(d.abs().max()) == 0.0          # the sub-gradient 0, never inf / NaN


# ---------------------------------------------------------------------------------------------- activations at their tails
ACTS = [None, "gelu", "tanh", "sigmoid", "relu", "softplus", "ELU", "silu"]


def _act_grid():
    """16 384 points over [-30, 30], +-0, +-1e-6, 20 +- 1 ulp (the softplus switch), +-87, +-89, +-100 (expf saturates)."""
    lin = torch.linspace(-30.0, 30.0, 16384, dtype=torch.float64).float()
    t20 = torch.tensor(20.0)
    inf = torch.tensor(float("inf"))
    edge = torch.stack([t20, torch.nextafter(t20, inf), torch.nextafter(t20, -inf)])
    rest = torch.tensor([0.0, -0.0, 1e-6, -1e-6, 87.0, -87.0, 89.0, -89.0, 100.0, -100.0])
    return torch.cat([lin, edge, rest])


def _act64(act, pre, dy=None):
    """act(pre), dy * act'(pre) by autograd of the oracle's activation table, in pre's dtype."""
    from oracle import transolver_oracle as orc
    if act is None:
        return pre.clone(), torch.ones_like(pre) if dy is None else dy.clone()
    x = pre.detach().clone().requires_grad_(True)
    y = orc._ACTS[act](x)
    y.backward(torch.ones_like(x) if dy is None else dy)
    return y.detach(), x.grad


def _act_bounds(act, pre_c, dy_c):
    """(yardstick, tau, fp64 act') of the act_bwd check: the fp32 CPU backward against the fp64 one, over |dy| (1 + |act'|)."""
    _, da = _act64(act, pre_c.double())
    _, r64 = _act64(act, pre_c.double(), dy_c.double())
    _, r32 = _act64(act, pre_c, dy_c)
    scale = dy_c.double().abs() * (1.0 + da.abs())
    yard = _yard(r32, r64, scale)
    return yard, _tau(yard), da


@pytest.mark.parametrize("act", ACTS)
def test_act_bwd_at_the_tails(act):
    from transformerbasednavierstokesolver_amd import ops
    grid = _act_grid()
    gen = torch.Generator().manual_seed(11)
    big = 8192 * 256 + 3
    for tag, pre_c in (("grid", grid), ("n=1", torch.tensor([-0.75])), ("second trip", grid.repeat(-(-big // grid.numel()))[-big:])):
        n = pre_c.numel()
        dy_c = torch.randn(n, generator=gen)
        dy_c[:: 7] = 1.0
        yard, tau, da = _act_bounds(act, pre_c, dy_c)
        (pbuf, pre), (dbuf, dy) = _banded(pre_c.to(DEV)), _banded(dy_c.to(DEV))
        out = poisoned(ops.act_bwd, dy, pre, act)
        assert _bands_untouched(pbuf, n) and _bands_untouched(dbuf, n)
        _, ref = _act64(act, pre.double(), dy.double())
        a = dy.double().abs() * (tau + (GELU_PHI_ABS if act == "gelu" else 0.0))
        frac = check_abs_rel(out, ref, a, tau, f"act_bwd {act} {tag}", n_flat=n, grid=min(8192, -(-n // 256)), vec=1)
        print(f"act_bwd {act} {tag}: fraction of the bound {frac:.3f}, tau {tau:.3e}, yardstick {yard:.3e}")
        _note(f"act_bwd {act}", frac * tau, tau, yard, tag)
        if tag == "grid":          # the kinks and the switch, written out (dy = 1 at index 0 mod 7 only: divide it out)
            d = (out / dy).cpu()
            at = {float(x): i for i, x in enumerate(pre_c.tolist())}
            zeros = [i for i, x in enumerate(pre_c.tolist()) if x == 0.0]
            assert len(zeros) == 2
            if act == "relu":
                assert all(float(d[i]) == 0.0 for i in zeros)
            if act == "ELU":
                assert all(float(d[i]) == 1.0 for i in zeros)
            if act == "softplus":
                up = float(torch.nextafter(torch.tensor(20.0), torch.tensor(float("inf"))))
                assert float(d[at[up]]) == 1.0 and float(d[at[100.0]]) == 1.0 and float(d[at[20.0]]) < 1.0 + 1e-6
            assert bool(torch.isfinite(out).all())


EPI_CASES = [(257, 64, "f32"), (257, 64, "split"), (32768, 128, "split")]       # the last: the row-stationary kernel


@pytest.mark.parametrize("M,K,engine", EPI_CASES)
@pytest.mark.parametrize("act", ACTS)
def test_epilogue_activations_at_the_tails(M, K, engine, act):
    """linear_fwd with an identity weight: y and the saved derivative against fp64 act / act' of the pre-activation the
    kernel itself returned, so the GEMM's rounding is out of the comparison.  act = None: there is no derivative to save,
    both calls return the pre-activation itself, which is y."""
    from transformerbasednavierstokesolver_amd import ops
    grid = _act_grid()
    assert M * K >= grid.numel()
    x = grid.repeat(-(-M * K // grid.numel()))[:M * K].reshape(M, K).to(DEV).contiguous()
    w = torch.eye(K, device=DEV)
    y, pre = poisoned(ops.linear_fwd, x, w, None, act=act, want_pre=True, engine=engine)
    y2, d = poisoned(ops.linear_fwd, x, w, None, act=act, want_pre=True, engine=engine, save_derivative=True)
    assert torch.equal(y, y2)
    assert float((pre - x).abs().max()) <= 1e-5, "an identity weight returns the grid as the pre-activation"
    if act is None:
        assert torch.equal(y, pre) and torch.equal(d, pre)
        return
    ry, rd = _act64(act, pre.double())
    pc = pre.cpu()
    y32, d32 = _act64(act, pc)
    tag = f"epilogue {act} M={M} K=N={K} {engine}"
    for name, got, ref, y32_, extra in (("y", y, ry, y32, GELU_PHI_ABS * pre.double().abs()), ("act'", d, rd, d32, GELU_PHI_ABS)):
        yard = _yard(y32_, ref.cpu(), 1.0 + ref.cpu().abs())
        tau = _tau(yard)
        a = tau + (extra if act == "gelu" else 0.0)
        frac = check_abs_rel(got, ref, a, tau, f"{tag} {name}")
        print(f"{tag} {name}: fraction of the bound {frac:.3f}, tau {tau:.3e}, yardstick {yard:.3e}")
        _note(f"epilogue {name} {act}", frac * tau, tau, yard, tag)


@pytest.mark.parametrize("engine", ["f32", "split"])
def test_linear_fn_route(engine):
    """functional.linear (LinearFn): act_bwd, then weight and data gradients, against fp64 autograd of the same layer."""
    from transformerbasednavierstokesolver_amd import functional as Fn
    M, K, N, act = 333, 76, 128, "silu"
    rng = np.random.default_rng(333)
    x, w, b, dy = (torch.from_numpy(rng.standard_normal(s).astype(np.float32) * f).to(DEV)
                   for s, f in (((M, K), 1.0), ((N, K), K ** -0.5), ((N,), 0.1), ((M, N), 1.0)))
    xg, wg, bg = (t.clone().requires_grad_(True) for t in (x, w, b))
    y = Fn.linear(xg, wg, bg, act, engine=engine)
    y.backward(dy)
    torch.cuda.synchronize()
    xd, wd, bd, dyd = (t.double() for t in (x, w, b, dy))
    lin, lin_abs = xd @ wd.t() + bd, xd.abs() @ wd.abs().t() + bd.abs()
    a, da = _act64(act, lin)
    d2, d2_abs = dyd * da, dyd.abs() * da.abs().clamp_min(1.0)      # act' holds to an absolute accuracy (test_gpu_elementwise)
    tag = f"LinearFn M={M} K={K} N={N} {act} {engine}"
    worst = [check_products(y.detach(), a, 1.13 * lin_abs + a.abs(), TAU[(engine, "fwd")], label=tag + " y"),
             check_products(xg.grad, d2 @ wd, d2_abs @ wd.abs(), TAU[(engine, "fwd")], label=tag + " dx"),
             check_products(wg.grad, d2.t() @ xd, d2_abs.t() @ xd.abs(), TAU[(engine, "wgrad")], label=tag + " dw"),
             check_products(bg.grad, d2.sum(0), d2_abs.sum(0), TAU[(engine, "wgrad")], label=tag + " db")]
    print(f"{tag}: y {worst[0]:.3e}, dx {worst[1]:.3e} (tau {TAU[(engine, 'fwd')]:.1e}); dw {worst[2]:.3e}, db {worst[3]:.3e} "
          f"(tau {TAU[(engine, 'wgrad')]:.1e})")
    _note(f"LinearFn fwd {engine}", max(worst[:2]), TAU[(engine, "fwd")], None, tag)
    _note(f"LinearFn wgrad {engine}", max(worst[2:]), TAU[(engine, "wgrad")], None, tag)
