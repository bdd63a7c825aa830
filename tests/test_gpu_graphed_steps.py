"""The captured one-call iterations on the GPU: harness.GraphedCallStep behind fit_darcy / fit_static / fit_plas
(graphed=True) and train.py --graphed, and the AdamW kernel that reads its coefficients from device memory.

No tolerance anywhere: a replay runs the kernels of the eager iteration in the same order on the same values, and
pa2d_adamw_step_dev shares its per-element device function with pa2d_adamw_step, so every comparison asks for equality.

Shapes are the fixtures' own tiny ones (tests/driver_restatement.py, tests/benchmark_restatement.py), with batch sizes
that give every epoch at least one full batch (a replay) and one short one (the eager step): Darcy 6 samples / batch 4,
plasticity 3 / 2, elasticity 40 / 16, airfoil and pipe cut to 10 samples / batch 4 (pipe's 9 x 9 mesh: odd row lengths)."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import benchmark_restatement as br
import driver_restatement as dr
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BETA2, EPS, WD = 0.999, 1e-8, 1e-5
GUARD, POISON = 64, 12345.0          # floats on either side of every buffer (a multiple of 4: the payload stays 16-byte aligned)
WARMUP = 2                           # GraphedCallStep's default number of warm-up iterations


# ------------------------------------------------------------------------------------------ the device-row AdamW kernel
def _banded(payload):
    """`payload` [n] inside a poisoned buffer: (whole buffer, the view the kernels get)."""
    n = payload.numel()
    buf = torch.full((GUARD + n + GUARD,), POISON, dtype=torch.float32, device=DEV)
    buf[GUARD:GUARD + n] = payload
    return buf, buf[GUARD:GUARD + n]


def _bands_untouched(buf, n):
    return bool((buf[:GUARD] == POISON).all()) and bool((buf[GUARD + n:] == POISON).all())


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("n", [4099, 3])          # a vector body with a 3-element tail; a tail alone
def test_device_row_adamw_equals_the_argument_form_bit_for_bit(n, clip):
    from transformerbasednavierstokesolver_amd import ops
    gen = torch.Generator().manual_seed(100 + n)
    p0 = torch.randn(n, generator=gen).to(DEV)
    bufs = {}
    for form in ("arg", "dev"):
        bufs[form] = [_banded(t) for t in (p0, torch.zeros(n, device=DEV), torch.zeros(n, device=DEV))]
    max_norm = 0.1 if clip else 0.0
    # two consecutive steps at the two ends of a OneCycle: lr and beta1 both change
    for step, (lr, beta1) in enumerate([(4e-5, 0.95), (1e-3, 0.85)], start=1):
        gbuf, g = _banded(torch.randn(n, generator=gen).to(DEV))
        gn = ops.sumsq(g) if clip else None
        if clip:
            assert float(gn.sqrt()) > 10 * max_norm                 # the clip bites
        (_, p), (_, m), (_, v) = bufs["arg"]
        ops.adamw_step(p, g, m, v, lr, beta1, BETA2, EPS, WD, step, gn, max_norm)
        row = ops.adamw_coefficients(lr, beta1, BETA2, EPS, WD, step, max_norm).to(DEV)
        (_, p), (_, m), (_, v) = bufs["dev"]
        ops.adamw_step_dev(p, g, m, v, row, gn)
        assert _bands_untouched(gbuf, n)
        for (ba, ta), (bd, td), name in zip(bufs["arg"], bufs["dev"], "pmv"):
            assert torch.equal(ta, td), (name, step, float((ta - td).abs().max()))
            assert _bands_untouched(ba, n) and _bands_untouched(bd, n), (name, step)
    assert not torch.equal(bufs["dev"][0][1], p0) and bool(torch.isfinite(bufs["dev"][0][1]).all())


def test_device_row_adamw_refuses_a_misaligned_row():
    from transformerbasednavierstokesolver_amd import ops
    t = [torch.zeros(8, device=DEV) for _ in range(4)]
    rows = torch.zeros(12, device=DEV)
    with pytest.raises(RuntimeError, match="PA2D_ERR_ARG"):
        ops.adamw_step_dev(*t, rows[1:9])
    torch.cuda.synchronize()
    assert all(float(x.abs().sum()) == 0.0 for x in t)


# ------------------------------------------------------------------------------------------ the loops
CASES = ("darcy", "airfoil", "pipe", "elas", "plas")
CUT = {"airfoil": (10, 4), "pipe": (10, 4)}          # (training samples kept, batch size)


def _hip_model(case):
    from transformerbasednavierstokesolver_amd import harness
    from transformerbasednavierstokesolver_amd.model import Transolver_Irregular_Mesh
    if case == "darcy":
        return harness.build_model(dr.model_config(case), dr.weights(case), DEV)
    cfg, sd = br.model_config(case), br.weights(case)
    if case != "elas":
        return harness.build_model(cfg, sd, DEV)
    m = Transolver_Irregular_Mesh.Model(space_dim=2, n_layers=cfg["n_layers"], n_hidden=cfg["n_hidden"], dropout=0.0,
                                        n_head=cfg["n_head"], Time_Input=False, mlp_ratio=cfg["mlp_ratio"], fun_dim=0,
                                        out_dim=1, slice_num=cfg["slice_num"], ref=cfg["ref"], unified_pos=cfg["unified_pos"])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.to(DEV)


def _initial_weights(case):
    return dr.weights(case) if case == "darcy" else br.weights(case)


@functools.lru_cache(maxsize=None)
def _setup(case):
    """(argv dict, data dict, epoch orders, time orders or None, samples per epoch, batch size): made once per case, shared
    by the eager and the graphed run and never written to (the loops copy what they move to the device)."""
    if case == "darcy":
        a, fx = dr.parse_argv(dr.CASES[case]["argv"]), dr.Fixture(case)
        return a, dr.darcy_data(case), fx.perms, None, dr.CASES[case]["ntrain"], a["batch_size"]
    a, fx, d = br.parse_argv(br.CASES[case]["argv"]), br.Fixture(case), br.load_data(case)
    n, bs, perms = br.seen_train(case), a["batch_size"], fx.perms
    if case in CUT:
        n, bs = CUT[case]
        d = dict(d, x_train=d["x_train"][:n], y_train=d["y_train"][:n])
        perms = [[i for i in p if i < n] for p in perms]
    return a, d, perms, fx.time_perms, n, bs


def _optimizer(case, model):
    from transformerbasednavierstokesolver_amd.optim import FusedAdamW
    a, _, _, _, n, bs = _setup(case)
    opt = FusedAdamW(model.parameters(), lr=a["lr"], weight_decay=a["weight_decay"], max_grad_norm=a["max_grad_norm"])
    if case == "darcy":
        return opt, dr.one_cycle(opt, case)
    if case == "elas":
        return opt, torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=a["epochs"])
    return opt, torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=a["lr"], epochs=a["epochs"], steps_per_epoch=-(-n // bs))


def _fit(case, model, opt, sched, graphed):
    from transformerbasednavierstokesolver_amd import harness
    from transformerbasednavierstokesolver_amd.utils.testloss import FusedTestLoss
    a, d, perms, time_perms, _, bs = _setup(case)
    common = dict(epochs=a["epochs"], batch_size=bs, loss_fn=FusedTestLoss(size_average=False), epoch_orders=perms,
                  grad_sync=opt.sync, graphed=graphed)
    if case == "darcy":
        return harness.fit_darcy(model, opt, sched, d, **common)
    if case == "plas":
        return harness.fit_plas(model, opt, sched, d, time_orders=time_perms, **common)
    return harness.fit_static(model, opt, sched, d, scheduler_per_epoch=case == "elas", **common)


@pytest.mark.parametrize("case", CASES)
def test_graphed_loop_is_bit_identical_to_the_eager_loop_and_replays(case, monkeypatch):
    a, _, perms, _, n, bs = _setup(case)
    per_iteration = br.PLAS_T if case == "plas" else 1          # model calls (and optimizer steps) per batch
    nfull, nshort = n // bs, int(n % bs > 0)
    assert nfull >= 1 and nshort == 1 and all(len(p) == n for p in perms)

    replays, train_calls = [0], [0]
    real_replay = torch.cuda.CUDAGraph.replay

    def replay(self):
        replays[0] += 1
        return real_replay(self)

    def count(module, args):
        train_calls[0] += int(module.training)

    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", replay)
    runs = []
    for graphed in (False, True):
        model = _hip_model(case)
        opt, sched = _optimizer(case, model)
        replays[0], train_calls[0] = 0, 0
        model.register_forward_pre_hook(count)
        hist = _fit(case, model, opt, sched, graphed)
        runs.append(dict(hist=hist, params={k: v.detach().clone() for k, v in model.state_dict().items()}, steps=opt.steps,
                         sched=sched.last_epoch, saved_steps=opt.state_dict()["fused"]["steps"], replays=replays[0],
                         train_calls=train_calls[0], exp_avg=opt.exp_avg.clone(), exp_avg_sq=opt.exp_avg_sq.clone()))
    eager, graph = runs
    iterations = a["epochs"] * (nfull + nshort) * per_iteration
    assert eager["replays"] == 0 and eager["train_calls"] == iterations == eager["steps"]
    # every full batch was served by a replay; Python ran the model for the warm-up, the capture and the short batches only
    assert graph["replays"] == a["epochs"] * nfull * per_iteration
    assert graph["train_calls"] == WARMUP + 1 + a["epochs"] * nshort * per_iteration != iterations
    # the same run, bit for bit
    assert graph["hist"] == eager["hist"], (eager["hist"], graph["hist"])
    bad = [k for k in eager["params"] if not torch.equal(eager["params"][k], graph["params"][k])]
    assert not bad, bad
    assert torch.equal(eager["exp_avg"], graph["exp_avg"]) and torch.equal(eager["exp_avg_sq"], graph["exp_avg_sq"])
    assert graph["steps"] == eager["steps"] == graph["saved_steps"] and graph["sched"] == eager["sched"]
    init = _initial_weights(case)
    assert any(not torch.equal(graph["params"][k].cpu(), torch.from_numpy(init[k])) for k in init)      # it did train
    assert all(np.isfinite(v) for h in graph["hist"] for v in h.values())


def test_a_changed_active_range_raises():
    """Darcy passes fx, so `placeholder` gets no gradient and lies outside the captured AdamW ranges; marking it as touched
    afterwards changes the optimizer's active ranges, and the next call refuses to replay."""
    from transformerbasednavierstokesolver_amd import harness
    case = "darcy"
    a, d, _, _, _, bs = _setup(case)
    model = _hip_model(case)
    opt, sched = _optimizer(case, model)
    _, yn, train, _, positions = harness._darcy_setup(model, d)
    fx, y = next(train.batches(bs))
    before = [p.detach().clone() for p in model.parameters()]
    step = harness.GraphedCallStep(model, opt, sched, (positions(bs), fx.clone(), y.clone()),
                                   harness._darcy_body(yn, d["dx"], d["s"]))
    # warm-up and capture left no trace: weights, moments, step count
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), before))
    assert opt.steps == 0 and float(opt.exp_avg.abs().sum()) == 0.0 == float(opt.exp_avg_sq.abs().sum())
    i = opt.sync.index_of(model.placeholder)
    assert not opt.sync.touched[i] and model.placeholder.grad is None
    loss, l2, deriv = step(None, fx, y)
    assert opt.steps == 1 and sched.last_epoch == 1 and all(bool(torch.isfinite(t)) for t in (loss, l2, deriv))
    assert any(not torch.equal(p, q) for p, q in zip(model.parameters(), before))
    opt.sync.touched[i] = True
    with pytest.raises(RuntimeError, match="re-capture"):
        step(None, fx, y)
    assert opt.steps == 1 and sched.last_epoch == 1          # refused before anything was staged


def test_train_command_line_end_to_end_pipe_graphed(tmp_path):
    """`python -m ...train --driver pipe --graphed 1` as a fresh child process on the Pipe_{X,Y,Q}.npy of br.write_files
    (the 129 x 129 mesh strided to 9 x 9; 20 training samples at batch 8: two replayed batches and a short eager one per
    epoch, clipped at 0.1 inside the optimizer); a second child reads the checkpoint with --eval 1 and prints the metric of
    the last epoch's test pass."""
    folder = br.write_files("pipe", str(tmp_path))
    common = [sys.executable, "-m", "transformerbasednavierstokesolver_amd.train", "--driver", "pipe", "--data_path", folder,
              "--ntrain", "20", "--ntest", "6", "--gpu", "0", "--save_name", "cli_pipe_graphed", "--batch-size", "8",
              "--epochs", "2", "--downsamplex", "16", "--downsampley", "16", "--max_grad_norm", "0.1", "--graphed", "1"] + br.MODEL_2D
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = subprocess.run(common, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert len([ln for ln in lines if re.match(r"Epoch \d+ Train loss : \d+\.\d{5}$", ln)]) == 2
    errs = [float(ln.split(":", 1)[1]) for ln in lines if ln.startswith("rel_err:")]
    ckpt = tmp_path / "checkpoints" / "cli_pipe_graphed.pt"
    assert len(errs) == 2 and os.path.isfile(ckpt)
    ev = subprocess.run(common + ["--eval", "1"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert ev.returncode == 0, ev.stderr[-2000:]
    last = ev.stdout.strip().splitlines()[-1]
    assert last.startswith("rel_err:")
    shown = float(last.split(":", 1)[1])
    assert np.isfinite(shown) and abs(shown - errs[-1]) <= 1e-5 + 1e-5 * abs(errs[-1])
    sd = torch.load(ckpt, weights_only=True)
    assert set(sd) == set(br.weights("pipe"))
