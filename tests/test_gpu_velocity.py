"""The velocity-field trainers on the HIP path (tiny model throughout: 8 x 8 points, C = 32, 4 heads, M = 8, 2 layers).

* harness.fit_velocity / fit_velocity_unrolled / fit_unrolled_t with optim.FusedAdamW, FusedTestLoss and the default engine
  against the reference scripts' own main() (fixtures G25-G27), at the bounds of test_gpu_drivers.py: max(floor, 4 x the
  fixture's own deviation) with floors 1e-5 on loss calls and metrics, 1e-5 rel-L2 on final parameters (2e-3 for to_q /
  to_k).  The training losses must have gone through functional.rel_l2_window and the test passes through
  pa2d_rollout_tail / pa2d_rollout_score (counted).
* harness.scored_rollout: its kept prediction equals the torch loop's (harness.rollout) bit for bit, and its scores are the
  torch loop's statement, ||pred_s - y_s|| / ||y_s|| per step and of the whole trajectory, evaluated in fp64 on those
  predictions, within the bound DERIVED in test_gpu_window.py from the kernel's addition depth: N = 64 points, k = 2:
  ntiles = 1, T = 1, tau_ratio = ((T + 12) / 2 + 1) + ((T + 10) / 2 + 1) + 1 = 15 u = 8.9e-7.
* GraphedScoredRollout against the eager scored_rollout, and each loop with graphed=True against the same loop eager, bit
  for bit, across look-ahead changes, with a short last batch (eager) in every epoch.
* `python -m ...train_velocity` end to end on synthetic data in a fresh child process under its own timeout."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import driver_restatement as dr
import velocity_restatement as vr
from conftest import ROOT
from elementwise_check import EPS32, check_abs_rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSS_FLOOR, PARAM_FLOOR, QK_FLOOR = 1e-5, 1e-5, 2e-3
FIT = {"velocity": "fit_velocity", "velocity_unrolled": "fit_velocity_unrolled", "unrolled_t": "fit_unrolled_t"}


def _module(case):
    """The HIP model of the case (the SOL wrapper for the unrolled drivers) with the fixture's initial weights, and the
    module whose state_dict the fixture holds."""
    from transformerbasednavierstokesolver_amd import harness
    from transformerbasednavierstokesolver_amd.model.SOL_Transolver_Structured_Mesh_2D import SOL_Transolver_Structured_Mesh_2D
    cfg = vr.model_config(case)
    if vr.CASES[case]["driver"] == "velocity":
        model = harness.build_model(cfg, vr.weights(case), DEV)
        return model, model
    sol = SOL_Transolver_Structured_Mesh_2D(
        space_dim=2, n_layers=cfg["n_layers"], n_hidden=cfg["n_hidden"], dropout=0.0, n_head=cfg["n_head"], Time_Input=False,
        mlp_ratio=cfg["mlp_ratio"], fun_dim=cfg["fun_dim"], out_dim=vr.STEP, slice_num=cfg["slice_num"], ref=cfg["ref"],
        unified_pos=cfg["unified_pos"], H=cfg["H"], W=cfg["W"], step=vr.STEP, look_ahead=1)
    sol.transolver_model.load_state_dict({k: torch.from_numpy(v) for k, v in vr.weights(case).items()}, strict=True)
    sol = sol.to(DEV)
    return sol, sol.transolver_model


def _fused(module, case, epochs=None, steps_per_epoch=None):
    from transformerbasednavierstokesolver_amd.optim import FusedAdamW
    from transformerbasednavierstokesolver_amd.utils.testloss import FusedTestLoss
    c, a = vr.CASES[case], vr.parse_argv(vr.CASES[case]["argv"])
    opt = FusedAdamW(module.parameters(), lr=a["lr"], weight_decay=a["weight_decay"])
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=a["lr"], epochs=epochs or a["epochs"],
                                                steps_per_epoch=steps_per_epoch or -(-c["ntrain"] // a["batch_size"]))
    return a, opt, sched, FusedTestLoss(size_average=False)


def _counted(monkeypatch, module, name):
    hits = []
    real = getattr(module, name)
    monkeypatch.setattr(module, name, lambda *a, **k: (hits.append(1), real(*a, **k))[1])
    return hits


@pytest.mark.parametrize("case", list(vr.CASES))
def test_fit_loops_on_the_hip_path(case, monkeypatch):
    from transformerbasednavierstokesolver_amd import functional, harness, ops
    fx = vr.Fixture(case)
    s = vr.script(case)
    module, held = _module(case)
    a, opt, sched, loss_fn = _fused(module, case)
    train_set, test_set = vr.datasets(case, DEV)
    window_calls, tails, scores = (_counted(monkeypatch, functional, "rel_l2_window"), _counted(monkeypatch, ops, "rollout_tail"),
                                   _counted(monkeypatch, ops, "rollout_score"))
    calls = []
    hist = getattr(harness, FIT[case])(module, opt, sched, train_set, test_set, epochs=a["epochs"], batch_size=a["batch_size"],
                                       T=s["T"], loss_fn=loss_fn, epoch_orders=fx.perms, grad_sync=opt.sync, calls=calls)
    if case != "velocity":
        assert [h["look_ahead"] for h in hist] == vr.LOOK_AHEAD_HISTORY[case]
    dr.check_scalars(vr.calls_of(calls), fx.calls, fx.calls_dev, LOSS_FLOOR, case + " loss calls")
    dr.check_scalars(dr.history_table(hist, fx.metric_names), fx.metrics, fx.metrics_dev, LOSS_FLOOR, case + " metrics")
    worst = dr.check_params(held.state_dict(), fx, PARAM_FLOOR, QK_FLOOR, label=case)
    print(case, "worst parameter rel-L2:", max(worst.items(), key=lambda kv: kv[1]))
    # every training loss on the window kernel, every test pass on the fused tail
    c = vr.CASES[case]
    nb_train, nb_test, S = -(-c["ntrain"] // a["batch_size"]), -(-c["ntest"] // a["batch_size"]), s["T"] // vr.STEP
    per_batch = S if case == "velocity" else None
    want = sum(nb_train * (per_batch or vr.train_calls(case, la)) for la in vr.look_ahead_history(case))
    assert len(window_calls) == want and len(tails) == a["epochs"] * nb_test * S and len(scores) == a["epochs"] * nb_test


def _fp64_scores(pred, yy, step):
    """(step_ratio [S, B], full_ratio [B]): the test pass's statement in fp64 on the CPU."""
    p, y = pred.double().cpu(), yy.double().cpu()
    B, _, T = y.shape
    norm = lambda t: t.reshape(B, -1).norm(dim=1)
    steps = torch.stack([norm(p[..., t:t + step] - y[..., t:t + step]) / norm(y[..., t:t + step]) for t in range(0, T, step)])
    return steps, norm(p - y) / norm(y)


@pytest.mark.parametrize("case", ["velocity", "velocity_unrolled"])
def test_scored_rollout_is_the_torch_loop_and_graphed_is_bit_identical(case):
    """T = 10 over a window of 10 columns (5 steps) and T = 20 over a window of 20 (10 steps)."""
    from transformerbasednavierstokesolver_amd import harness
    s = vr.script(case)
    _, model = _module(case)
    model.eval()
    _, test_set = vr.datasets(case, DEV)
    batches = list(test_set.batches(2))
    x, fx, yy = batches[0]
    fx0 = fx.clone()
    step_ratio, full_ratio, pred = harness.scored_rollout(model, x, fx, yy, vr.STEP, keep_pred=True)
    assert torch.equal(fx, fx0) and pred.shape == yy.shape and step_ratio.shape == (s["T"] // vr.STEP, 2)
    assert torch.equal(pred, harness.rollout(model, x, fx, s["T"] // vr.STEP, step=vr.STEP))      # the torch loop's frames
    again = harness.scored_rollout(model, x, fx, yy, vr.STEP)
    assert again[2] is None and torch.equal(again[0], step_ratio) and torch.equal(again[1], full_ratio)
    want_steps, want_full = _fp64_scores(pred, yy, vr.STEP)
    tau = 15 * EPS32                                         # derived: see the module docstring
    for name, got, ref in (("step_ratio", step_ratio, want_steps), ("full_ratio", full_ratio, want_full)):
        frac = check_abs_rel(got, ref, 0.0, tau * (1 + tau), f"scored_rollout {case} {name}")
        print(f"scored_rollout {case} {name}: measured {frac * tau:.3e}, derived bound {tau:.3e}")
    # the whole rollout from ONE graph: the same bits, also on another batch content and after the weights moved
    graph = harness.GraphedScoredRollout(model, x, fx, yy, vr.STEP, keep_pred=True)
    for k, (bx, bfx, byy) in enumerate([(x, fx, yy), (x, fx.flip(0), yy.flip(0)), (x, fx, yy)]):
        if k == 2:
            with torch.no_grad():
                for p in model.parameters():
                    p.mul_(1.0 + 2.0 ** -7)
        eager = harness.scored_rollout(model, bx, bfx, byy, vr.STEP, keep_pred=True)
        replay = graph.run(bx, bfx, byy)
        for name, a, b in zip(("step_ratio", "full_ratio", "pred"), eager, replay):
            assert torch.equal(a, b), f"GraphedScoredRollout {case} run {k}: {name} differs from the eager rollout"
    assert not torch.equal(eager[2], pred)                   # the moved weights were seen


@pytest.mark.parametrize("case", list(vr.CASES))
def test_graphed_loops_are_bit_identical_to_eager(case):
    """5 epochs with a curriculum period of 2 (look-ahead 1, 1, 2, 2, 3: two graphs are built on the way, the third value
    too); ntrain = 3 at batch 2: a replayed full batch and an eager short batch in every epoch; the test pass of 3 samples
    likewise replays one batch and runs one eagerly."""
    from transformerbasednavierstokesolver_amd import harness
    s, epochs = vr.script(case), 5
    from transformerbasednavierstokesolver_amd import data
    train_full, test_set = vr.datasets(case, DEV)
    train_set = data.ResidentDataset(*[t[:3] for t in train_full.tensors])
    rng = np.random.default_rng(31)
    orders = [rng.permutation(3).tolist() for _ in range(epochs)]
    runs = []
    for graphed in (False, True):
        module, held = _module(case)
        a, opt, sched, loss_fn = _fused(module, case, epochs, steps_per_epoch=2)
        calls = []
        kw = {} if case == "velocity" else dict(period=2)
        hist = getattr(harness, FIT[case])(module, opt, sched, train_set, test_set, epochs=epochs, batch_size=2, T=s["T"],
                                           loss_fn=loss_fn, epoch_orders=orders, grad_sync=opt.sync, graphed=graphed,
                                           calls=calls, **kw)
        runs.append((hist, vr.calls_of(calls), {k: v.detach().clone() for k, v in held.state_dict().items()}))
    (h0, c0, p0), (h1, c1, p1) = runs
    if case != "velocity":
        assert [h["look_ahead"] for h in h0] == [1, 1, 2, 2, 3]
    assert h0 == h1, (h0, h1)
    assert np.array_equal(c0, c1), np.flatnonzero(c0 != c1)[:8]
    assert all(torch.equal(p0[k], p1[k]) for k in p0), [k for k in p0 if not torch.equal(p0[k], p1[k])]
    assert any(not torch.equal(p0[k].cpu(), torch.from_numpy(vr.weights(case)[k])) for k in p0)     # it did train


def test_train_velocity_command_line_end_to_end(tmp_path):
    """`python -m ...train_velocity --driver unrolled_t --graphed 1` on synthetic data as a fresh child process; a second
    child reads the checkpoint with --eval 1 and prints the last epoch's test metric."""
    common = [sys.executable, "-m", "transformerbasednavierstokesolver_amd.train_velocity", "--driver", "unrolled_t",
              "--data_path", "synthetic", "--ntrain", "3", "--ntest", "2", "--gpu", "0", "--save_name", "cli", "--batch-size", "2",
              "--epochs", "2"] + vr.TINY
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = subprocess.run(common + ["--graphed", "1"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("Epoch ")]
    assert len(lines) == 2 and os.path.isfile(tmp_path / "checkpoints" / "cli.pt")
    last = float(re.search(r"test_step_loss:([0-9.eE+-]+)", lines[-1]).group(1))
    ev = subprocess.run(common + ["--eval", "1"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert ev.returncode == 0, ev.stderr[-2000:]
    shown = float(re.search(r"test_step_loss:([0-9.eE+-]+)", ev.stdout.strip().splitlines()[-1]).group(1))
    assert np.isfinite(shown) and abs(shown - last) <= 1e-5 + 1e-5 * abs(last)
    sd = torch.load(tmp_path / "checkpoints" / "cli.pt", weights_only=True)
    assert set(sd) == set(vr.weights("unrolled_t"))            # the INNER model's keys
