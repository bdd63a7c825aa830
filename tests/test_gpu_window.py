"""csrc/pa2d_window.hip on the MI355X, element by element: the column-window relative L2 (pa2d_rel_l2_window_fwd / _bwd) and the
fused scored-rollout tail (pa2d_rollout_tail, pa2d_rollout_score), in the manner of test_gpu_step_tail_elementwise.py.

Copies.  The window after a tail call is cat(window[..., k:], pred) and the trajectory columns [c, c + k) are pred: both
must be EXACT.  The trajectory buffer, the record and a guard ring around the window are pre-filled with a sentinel
(0x71 bytes = 1.2e30); every element the call has no business with must still hold it afterwards.  Buffers that an op
allocates itself go through elementwise_check.poisoned (NaN, then 1.2e30; finite and bit-identical between the two runs).

Exact probes.  pred - y is 2^j at <= 10 positions and 0 elsewhere, y is 2^j at other positions: every partial sum of the
squares 4^j is an integer below 2^24, so the record's slot must add up to sum 4^j bit for bit in any order
(elementwise_check.decode_probe_sum names a probe that was dropped or counted twice), and dnorm^2 / ynorm^2 must be that
integer up to the rounding of one fp32 root (2^-22 relative; a dropped 4^0 is 2.9e-6).  The positions sit on the edges of
what a thread, a workgroup pass (256 / 1024 elements) and a 64-row tile cover, and in the tile that wraps round to workgroup 0.

Derived bounds (u = 2^-24; all terms are >= 0, so a value that passes through D roundings is off by at most D u (1 + D u)
relative).  Depth of a term's path to its sum:
  rel_l2_window_fwd_kernel: L = N k elements of a sample over nsplit = min(64, ceil(L / 1024)) workgroups of 256 threads:
  T = ceil(L / (256 nsplit)) adds per thread and 1 for the product (FMA contraction only removes roundings), 6 for the
  64-lane butterfly, 2 for (red0 + red1) + (red2 + red3); the records are added in double (nothing at this scale) and the
  sum is rounded to fp32 once: D_y = T + 10.  pred - y is rounded once before it is squared (2 more): D_d = T + 12.
  rollout_tail_kernel: ntiles = ceil(N / 64) row tiles over nsplit = min(64, ntiles) workgroups; a thread adds
  ceil(64 k / 256) terms per tile over ceil(ntiles / nsplit) tiles: T = ceil(ntiles / nsplit) ceil(k / 4); the rest as above.
  rollout_score_kernel adds the steps' sums in double and rounds once, so full_ratio has the depth of one step.
  The roots halve the relative error and round once: tau_yn = (D_y / 2 + 1) u, tau_dn = (D_d / 2 + 1) u; a quotient:
  tau_ratio = tau_dn + tau_yn + u (ratio, step_ratio, full_ratio).
  dpred = s (pred - y), s = gout / (dnorm ynorm) from the kernel's own fp32 norms: the difference, the product of the norms,
  the quotient and the final product round once each: tau_bwd = tau_dn + tau_yn + 4 u, checked as tau_bwd |ref| per element.
At N = 4113, k = 8: window T = 4, tau_ratio = 9 u + 8 u + u = 18 u = 1.07e-6; tail T = 4, the same.  At N = 1: T = 1,
tau_ratio = 15 u = 8.9e-7.
Every bound is applied as tau (1 + tau) |ref|.
"""
import itertools

import numpy as np
import pytest
import torch

from elementwise_check import EPS32, check_abs_rel, decode_probe_sum, poisoned
from transformerbasednavierstokesolver_amd import _lib, ops
from transformerbasednavierstokesolver_amd import functional as Fn

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = float(np.frombuffer(bytes([0x71] * 4), dtype=np.float32)[0])
SPLIT = 64
BS, NS, KS = (1, 3), (1, 63, 4113), (1, 2, 3, 8)
WIDE = 21                                   # columns of the wider target tensor
_data = {}


def _case(B, N):
    """Seeded CPU tensors of one (B, N), made once and never changed: target [B, N, 23] and per k a pred [B, N, k]."""
    if (B, N) not in _data:
        g = torch.Generator().manual_seed(1000 * B + N)
        _data[B, N] = dict(yy=torch.randn(B, N, WIDE + 2, generator=g),
                           pred={k: torch.randn(B, N, k, generator=g) for k in KS},
                           win=torch.randn(B, N, 64, generator=g))
    return _data[B, N]


def _odd_aligned(t):
    """A GPU copy of `t` whose first element sits 4 bytes past a 16-byte boundary."""
    store = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    out = store[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4
    return out


def window_depth(N, k):
    L = N * k
    nsplit = min(SPLIT, -(-L // 1024))
    return -(-L // (256 * nsplit))


def tail_depth(N, k):
    ntiles = -(-N // 64)
    nsplit = min(SPLIT, ntiles)
    return -(-ntiles // nsplit) * -(-k // 4)


def taus(T):
    tau_yn, tau_dn = ((T + 10) / 2 + 1) * EPS32, ((T + 12) / 2 + 1) * EPS32
    return tau_dn, tau_yn, tau_dn + tau_yn + EPS32


def _ref_norms(pred, y):
    """fp64 (dnorm, ynorm) per sample of CPU tensors pred, y [B, N, k]."""
    B = pred.shape[0]
    p, t = pred.double().reshape(B, -1), y.double().reshape(B, -1)
    return (p - t).norm(dim=1), t.norm(dim=1)


def _check_rel(got, ref, tau, label):
    frac = check_abs_rel(got, ref, 0.0, tau * (1 + tau), label)
    print(f"{label}: measured {frac * tau:.3e}, derived bound {tau:.3e}")


def _probe_positions(N, k):
    L = N * k
    want = [0, 1, 255, 256, 1023, 1024, 63 * k, 64 * k, 64 * 64 * k, L - 1, L - 2, 64 * k - 1]
    out = []
    for q in want:
        if 0 <= q < L and q not in out:
            out.append(q)
    return out[:10]


def _probes(B, N, k):
    """(pred, y [B, N, k] CPU, positions of the difference probes, positions of the target probes): sample b's probes are
    the same positions (the sums are per sample)."""
    L = N * k
    dpos = _probe_positions(N, k)
    ypos = [(q + 7) % L for q in dpos]
    ypos = list(dict.fromkeys(ypos))
    d, y = torch.zeros(B, L), torch.zeros(B, L)
    for j, q in enumerate(dpos):
        d[:, q] = 2.0 ** j
    for j, q in enumerate(ypos):
        y[:, q] = 2.0 ** j
    return (y + d).view(B, N, k), y.view(B, N, k), dpos, ypos      # 2^i + 2^j is exact in fp32, so pred - y is the probe


# ---------------------------------------------------------------------------------------------- rel_l2_window
@pytest.mark.parametrize("B,N", list(itertools.product(BS, NS)))
def test_rel_l2_window_random_against_fp64(B, N):
    c = _case(B, N)
    yy_store = c["yy"].to(DEV)
    for k, (col0, view) in itertools.product(KS, ((5, "whole"), (None, "end"), (3, "view"))):
        yy = yy_store if view != "view" else yy_store[..., 1:1 + WIDE]           # a view: rows 23 apart, odd phase
        col0 = yy.shape[-1] - k if col0 is None else col0
        pred = _odd_aligned(c["pred"][k])
        dn, yn, ratio = poisoned(ops.rel_l2_window_fwd, pred, yy, col0)
        y_cpu = yy.cpu()[..., col0:col0 + k]
        rdn, ryn = _ref_norms(c["pred"][k], y_cpu)
        tau_dn, tau_yn, tau_ratio = taus(window_depth(N, k))
        tag = f"rel_l2_window_fwd B={B} N={N} k={k} col0={col0} {view}"
        _check_rel(dn, rdn, tau_dn, tag + " dnorm")
        _check_rel(yn, ryn, tau_yn, tag + " ynorm")
        _check_rel(ratio, rdn / ryn, tau_ratio, tag + " ratio")
        gout = torch.linspace(0.5, 1.5, B, device=DEV)
        dpred = poisoned(ops.rel_l2_window_bwd, pred, yy, col0, dn, yn, gout)
        ref = gout.cpu().double().view(B, 1, 1) * (c["pred"][k].double() - y_cpu.double()) / (rdn * ryn).view(B, 1, 1)
        tau = tau_dn + tau_yn + 4 * EPS32
        frac = check_abs_rel(dpred, ref, 0.0, tau * (1 + tau), tag + " dpred", n_flat=dpred.numel(), vec=1)
        print(f"{tag} dpred: measured {frac * tau:.3e}, derived bound {tau:.3e}")


@pytest.mark.parametrize("B,N,k", [(1, 1, 1), (3, 63, 3), (1, 4113, 2), (3, 4113, 8)])
def test_rel_l2_window_exact_probes_and_zero_difference(B, N, k):
    pred, y, dpos, ypos = _probes(B, N, k)
    yy = torch.full((B, N, WIDE), 3.0)
    yy[..., 7:7 + k] = y
    yy = yy.to(DEV)
    dn, yn, ratio = poisoned(ops.rel_l2_window_fwd, pred.to(DEV), yy, 7)
    for name, got, pos in (("dnorm", dn, dpos), ("ynorm", yn, ypos)):
        want = sum(4 ** j for j in range(len(pos)))
        sq = got.double().cpu() ** 2
        assert bool(((sq - want).abs() <= 2.0 ** -22 * want).all()), \
            f"B={B} N={N} k={k} {name}^2 = {sq.tolist()}, want {want}: " + decode_probe_sum(round(float(sq[0])), pos)[1]
    # pred == y: dnorm = 0, ratio = 0 and the zero sub-gradient, never inf / NaN
    same = yy[..., 7:7 + k].contiguous()
    dn, yn, ratio = poisoned(ops.rel_l2_window_fwd, same, yy, 7)
    assert torch.equal(dn, torch.zeros_like(dn)) and torch.equal(ratio, torch.zeros_like(ratio)) and bool((yn > 0).all())
    d = poisoned(ops.rel_l2_window_bwd, same, yy, 7, dn, yn, torch.ones(B, device=DEV))
    assert torch.equal(d, torch.zeros_like(d))


def test_rel_l2_window_autograd_equals_the_reshaped_loss():
    """functional.rel_l2_window: the value and the gradient of TestLoss.rel on the reshaped copy, in fp64 on the CPU."""
    B, N, k = 3, 63, 2
    c = _case(B, N)
    yy = c["yy"].to(DEV)
    pred = c["pred"][k].to(DEV).requires_grad_(True)
    loss = Fn.rel_l2_window(pred, yy, 5, k).sum()
    loss.backward()
    p64 = c["pred"][k].double().requires_grad_(True)
    y64 = c["yy"][..., 5:5 + k].double()
    ref = ((p64 - y64).reshape(B, -1).norm(dim=1) / y64.reshape(B, -1).norm(dim=1)).sum()
    ref.backward()
    tau_dn, tau_yn, tau_ratio = taus(window_depth(N, k))
    _check_rel(loss.detach(), ref.detach(), tau_ratio + (B - 1) * EPS32, "rel_l2_window summed")
    tau = tau_dn + tau_yn + 4 * EPS32
    check_abs_rel(pred.grad, p64.grad, 0.0, tau * (1 + tau), "rel_l2_window grad")
    assert yy.grad is None
    with pytest.raises(ValueError):
        Fn.rel_l2_window(pred, yy, 5, 3)
    with pytest.raises(ValueError):
        ops.rel_l2_window_fwd(pred.detach(), yy, WIDE + 1)


# ---------------------------------------------------------------------------------------------- rollout tail and score
def _guarded(t):
    """(store, view): a GPU copy of [B, N, F] `t` inside a sentinel-filled store, 9 guard floats in front of it and 8
    behind (so the window itself is only 4-byte aligned)."""
    store = torch.full((t.numel() + 17,), SENTINEL, dtype=torch.float32, device=DEV)
    out = store[9:9 + t.numel()].view(t.shape)
    out.copy_(t)
    return store, out


def _run_rollout(B, N, k, F, S, c0, tcol, Ttraj, seed_shift=0):
    """S tail calls and the score on fresh buffers.  Returns everything the checks read (GPU tensors) and the CPU inputs."""
    c = _case(B, N)
    yy = c["yy"].to(DEV)[..., 1:1 + WIDE]
    g = torch.Generator().manual_seed(77 + seed_shift)
    preds = [c["pred"][k]] + [torch.randn(B, N, k, generator=g) for _ in range(S - 1)]
    store, win = _guarded(c["win"][..., :F].contiguous())
    traj = torch.full((B, N, Ttraj), SENTINEL, dtype=torch.float32, device=DEV)
    record = torch.full((S + 1, B, SPLIT, 2), SENTINEL, dtype=torch.float32, device=DEV)     # slot S is never written
    wins = []
    for s, p in enumerate(preds):
        ops.rollout_tail(_odd_aligned(p), win, traj, tcol + s * k, yy, c0 + s * k, record, s)
        wins.append(win.clone())
    return dict(yy=yy, preds=preds, store=store, win=win, wins=wins, traj=traj, record=record, win0=c["win"][..., :F])


@pytest.mark.parametrize("B,N", list(itertools.product(BS, NS)))
def test_rollout_tail_copies_are_exact_and_scores_meet_the_derived_bound(B, N):
    for k in KS:
        for F in sorted({k, 10, 11, 64}):
            S = 2
            c0, tcol, Ttraj = 3, 5, 5 + S * k + 4             # odd offsets; a trajectory buffer wider than what is written
            r = _run_rollout(B, N, k, F, S, c0, tcol, Ttraj)
            tag = f"rollout_tail B={B} N={N} k={k} F={F}"
            # the window: shifted by k and pred appended, step after step; the guard ring untouched
            want = r["win0"].clone()
            for s, p in enumerate(r["preds"]):
                want = torch.cat((want[..., k:], p), dim=-1)
                assert torch.equal(r["wins"][s].cpu(), want), f"{tag}: window after step {s} is not the exact shifted copy"
            st = r["store"].cpu()
            assert bool((st[:9] == SENTINEL).all()) and bool((st[9 + want.numel():] == SENTINEL).all()), tag + ": guard ring"
            # the trajectory: the written columns are exact copies, every other column keeps the poison
            traj = r["traj"].cpu()
            assert torch.equal(traj[..., tcol:tcol + S * k], torch.cat(r["preds"], -1)), tag + ": trajectory columns"
            assert bool((traj[..., :tcol] == SENTINEL).all()) and bool((traj[..., tcol + S * k:] == SENTINEL).all()), \
                tag + ": trajectory columns outside [c, c + k) were written"
            # the record: the slots in use are finite, everything else keeps the poison
            ntiles = -(-N // 64)
            nsplit = min(SPLIT, ntiles)
            rec = r["record"].cpu()
            assert bool(torch.isfinite(rec[:S, :, :nsplit]).all()) and bool((rec[:S, :, :nsplit] != SENTINEL).all())
            assert bool((rec[:S, :, nsplit:] == SENTINEL).all()) and bool((rec[S] == SENTINEL).all()), tag + ": record"
            # the score against fp64
            step_ratio, full_ratio = poisoned(ops.rollout_score, r["record"][:S], N)
            yy_cpu = r["yy"].cpu()
            tau_ratio = taus(tail_depth(N, k))[2]
            d2 = y2 = 0
            for s, p in enumerate(r["preds"]):
                rdn, ryn = _ref_norms(p, yy_cpu[..., c0 + s * k:c0 + (s + 1) * k])
                _check_rel(step_ratio[s], rdn / ryn, tau_ratio, f"{tag} step_ratio[{s}]")
                d2, y2 = d2 + rdn ** 2, y2 + ryn ** 2
            _check_rel(full_ratio, (d2 / y2).sqrt(), tau_ratio, tag + " full_ratio")
            # ... which is the relative L2 of the concatenated prediction against the whole target
            fdn, fyn = _ref_norms(torch.cat(r["preds"], -1), yy_cpu[..., c0:c0 + S * k])
            _check_rel(full_ratio, fdn / fyn, tau_ratio, tag + " full_ratio (concatenated)")


@pytest.mark.parametrize("B,N,k,F", [(1, 1, 1, 1), (3, 63, 3, 10), (1, 4113, 2, 10), (3, 4113, 8, 64)])
def test_rollout_tail_exact_probes_and_second_call_same_bits(B, N, k, F):
    pred, y, dpos, ypos = _probes(B, N, k)
    yy = torch.full((B, N, WIDE), 3.0)
    yy[..., 9:9 + k] = y
    yy = yy.to(DEV)
    win0 = _case(B, N)["win"][..., :F].contiguous().to(DEV)
    outs = []
    for _ in range(2):
        win = win0.clone()
        record = torch.full((1, B, SPLIT, 2), SENTINEL, dtype=torch.float32, device=DEV)
        ops.rollout_tail(pred.to(DEV), win, None, 0, yy, 9, record, 0)
        outs.append((win, record, *ops.rollout_score(record, N)))
    for a, b in zip(*outs):
        assert torch.equal(a, b), "a second call on the same inputs gave other bits"
    nsplit = min(SPLIT, -(-N // 64))
    rec = outs[0][1][0, :, :nsplit].cpu().double().sum(1)                      # [B, 2]: integers below 2^24, exact in any order
    for col, pos, name in ((0, dpos, "sum d^2"), (1, ypos, "sum y^2")):
        for b in range(B):
            ok, text = decode_probe_sum(float(rec[b, col]), pos)
            assert ok, f"rollout_tail B={B} N={N} k={k} F={F} sample {b} {name}: {text}"
    # no target: the window and the trajectory are still served, the record is not touched
    win, record = win0.clone(), torch.full((1, B, SPLIT, 2), SENTINEL, dtype=torch.float32, device=DEV)
    traj = torch.full((B, N, k + 2), SENTINEL, dtype=torch.float32, device=DEV)
    ops.rollout_tail(pred.to(DEV), win, traj, 1, None, 0, record, 0)
    assert torch.equal(win, outs[0][0]) and torch.equal(traj[..., 1:1 + k].cpu(), pred)
    assert bool((record == SENTINEL).all()) and bool((traj[..., 0] == SENTINEL).all()) and bool((traj[..., -1] == SENTINEL).all())


def test_zero_difference_scores_zero():
    B, N, k, F = 3, 63, 2, 10
    c = _case(B, N)
    yy = c["yy"].to(DEV)
    record = ops.rollout_record(1, B, yy)
    ops.rollout_tail(yy[..., 4:4 + k].contiguous(), c["win"][..., :F].contiguous().to(DEV), None, 0, yy, 4, record, 0)
    step_ratio, full_ratio = poisoned(ops.rollout_score, record, N)
    assert torch.equal(step_ratio, torch.zeros_like(step_ratio)) and torch.equal(full_ratio, torch.zeros_like(full_ratio))


def test_unsupported_shapes_return_their_codes_before_any_pointer_is_read():
    """PA2D_ERR_UNSUPPORTED (1002) with NULL for every pointer; B = 0 / N = 0 return 0 and touch nothing; a pointer that is
    not 4-byte aligned is PA2D_ERR_ARG (1001)."""
    L = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    for k in (0, 9, -1):
        assert L.pa2d_rel_l2_window_fwd(0, 0, 21, 0, 0, 0, 0, 0, 0, 2, 64, k, st) == 1002
        assert L.pa2d_rel_l2_window_bwd(0, 0, 21, 0, 0, 0, 0, 0, 2, 64, k, st) == 1002
        assert L.pa2d_rollout_tail(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2, 64, k, 10, st) == 1002
    for k, F in ((3, 2), (2, 65), (8, 7)):
        assert L.pa2d_rollout_tail(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2, 64, k, F, st) == 1002
    assert L.pa2d_rel_l2_window_fwd(0, 0, 21, 0, 0, 0, 0, 0, 0, 65536, 64, 2, st) == 1002
    for B, N in ((0, 64), (2, 0)):
        assert L.pa2d_rel_l2_window_fwd(0, 0, 21, 0, 0, 0, 0, 0, 0, B, N, 2, st) == 0
        assert L.pa2d_rel_l2_window_bwd(0, 0, 21, 0, 0, 0, 0, 0, B, N, 2, st) == 0
        assert L.pa2d_rollout_tail(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, B, N, 2, 10, st) == 0
        assert L.pa2d_rollout_score(0, 0, 0, 1, B, N, st) == 0
    buf = torch.zeros(4096, device=DEV)
    p = buf.data_ptr()
    assert L.pa2d_rel_l2_window_fwd(p + 2, p, 2, 128, p, p, p, p, 4096, 1, 8, 2, st) == 1001
    assert L.pa2d_rel_l2_window_fwd(p, p, 2, 128, p, p, p, p, 16, 1, 8, 2, st) == 1003              # workspace too small
    assert L.pa2d_rollout_tail(p, p + 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 8, 2, 10, st) == 1001
    assert L.pa2d_rollout_tail(p, p, p, 4, 3, 0, 0, 0, 0, 0, 1, 1, 8, 2, 10, st) == 1001             # columns [3, 5) of 4
    torch.cuda.synchronize()
    assert bool((buf == 0).all())
    with pytest.raises(ValueError):
        ops.rollout_tail(torch.zeros(1, 8, 3, device=DEV), torch.zeros(1, 8, 2, device=DEV))
    with pytest.raises(ValueError):
        ops.rollout_tail(torch.zeros(1, 8, 2, device=DEV), torch.zeros(1, 8, 65, device=DEV))
