"""The epoch loops on the HIP path against the reference drivers' own main() (fixtures G14-G16): the HIP models (default
engine) with optim.FusedAdamW and FusedTestLoss through harness.fit_ns (both variants), fit_unrolled and
fit_darcy (fused Darcy loss).  Bounds: max(floor, 4 x the fixture's own deviation) with the project's fp32 floors, 1e-5 on
losses and metrics, 1e-5 rel-L2 on final parameters (2e-3 for to_q / to_k).  Then fit_ns(graphed=True) bit for bit against
the eager loop, and the command line end to end in a fresh child process."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import driver_restatement as dr
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSS_FLOOR, PARAM_FLOOR, QK_FLOOR = 1e-5, 1e-5, 2e-3


def _hip_model(case):
    from transformerbasednavierstokesolver_amd import harness
    return harness.build_model(dr.model_config(case), dr.weights(case), DEV)


def _fused_adamw(model, case, clip=True):
    from transformerbasednavierstokesolver_amd.optim import FusedAdamW
    a = dr.parse_argv(dr.CASES[case]["argv"])
    opt = FusedAdamW(model.parameters(), lr=a["lr"], weight_decay=a["weight_decay"],
                     max_grad_norm=a["max_grad_norm"] if clip else None)
    return a, opt, dr.one_cycle(opt, case)


def _recorder():
    from transformerbasednavierstokesolver_amd.utils.testloss import FusedTestLoss
    return dr.RecordingLoss(FusedTestLoss(size_average=False))


def _check(fx, calls, want_calls, want_dev, history, state_dict, label):
    dr.check_scalars(calls, want_calls, want_dev, LOSS_FLOOR, label + " loss calls")
    dr.check_scalars(dr.history_table(history, fx.metric_names), fx.metrics, fx.metrics_dev, LOSS_FLOOR, label + " metrics")
    worst = dr.check_params(state_dict, fx, PARAM_FLOOR, QK_FLOOR, label=label)
    print(label, "worst parameter rel-L2:", max(worst.items(), key=lambda kv: kv[1]))


@pytest.mark.parametrize("case", ["ns_up", "ns_clip"])
def test_fit_ns_on_the_hip_path(case):
    from transformerbasednavierstokesolver_amd import harness
    fx = dr.Fixture(case)
    model = _hip_model(case)
    a, opt, sched = _fused_adamw(model, case)
    train_set, test_set = dr.ns_datasets(case, DEV)
    rec = _recorder()
    hist = harness.fit_ns(model, opt, sched, train_set, test_set, epochs=a["epochs"], batch_size=a["batch_size"],
                          loss_fn=rec, epoch_orders=fx.perms, grad_sync=opt.sync)
    _check(fx, rec.values(), fx.calls, fx.calls_dev, hist, model.state_dict(), case)


def test_fit_unrolled_on_the_hip_path():
    from transformerbasednavierstokesolver_amd import harness
    from transformerbasednavierstokesolver_amd.model.SOL_Transolver_Structured_Mesh_2D import SOL_Transolver_Structured_Mesh_2D
    case = "unrolled"
    fx = dr.Fixture(case)
    cfg = dr.model_config(case)
    sol = SOL_Transolver_Structured_Mesh_2D(
        space_dim=2, n_layers=cfg["n_layers"], n_hidden=cfg["n_hidden"], dropout=0.0, n_head=cfg["n_head"], Time_Input=False,
        mlp_ratio=cfg["mlp_ratio"], fun_dim=cfg["fun_dim"], out_dim=1, slice_num=cfg["slice_num"], ref=cfg["ref"],
        unified_pos=cfg["unified_pos"], H=cfg["H"], W=cfg["W"], step=1, look_ahead=1)
    sol.transolver_model.load_state_dict({k: torch.from_numpy(v) for k, v in dr.weights(case).items()}, strict=True)
    sol = sol.to(DEV)
    a, opt, sched = _fused_adamw(sol, case, clip=False)
    train_set, test_set = dr.ns_datasets(case, DEV)
    rec = _recorder()
    hist = harness.fit_unrolled(sol, opt, sched, train_set, test_set, epochs=a["epochs"], batch_size=a["batch_size"],
                                loss_fn=rec, epoch_orders=fx.perms, grad_sync=opt.sync)
    assert [h["look_ahead"] for h in hist] == [1, 1, 2, 4]
    _check(fx, rec.values(), fx.calls, fx.calls_dev, hist, sol.transolver_model.state_dict(), case)


def test_fit_darcy_on_the_hip_path_with_the_fused_loss(monkeypatch):
    """The fused training loss never calls `loss_fn`, so the recorder sees the test-pass losses only: G16's per-call
    TRAINING losses are checked here through the epoch metrics `reg` and `train_loss` (same bound), not call by call;
    tests/test_drivers_host.py checks every call on the torch path."""
    from transformerbasednavierstokesolver_amd import functional, harness
    case = "darcy"
    fx = dr.Fixture(case)
    c = dr.CASES[case]
    model = _hip_model(case)
    a, opt, sched = _fused_adamw(model, case)
    fused_calls = []
    real = functional.darcy_loss
    monkeypatch.setattr(functional, "darcy_loss", lambda *args: (fused_calls.append(1), real(*args))[1])
    rec = _recorder()
    d = dr.darcy_data(case)
    hist = harness.fit_darcy(model, opt, sched, d, epochs=a["epochs"], batch_size=a["batch_size"],
                             loss_fn=rec, epoch_orders=fx.perms, grad_sync=opt.sync)
    assert d["y_normalizer"].mean.device.type == "cpu"            # the caller's normaliser stays where it was
    ev = harness.evaluate_darcy(model, d, a["batch_size"], _recorder())
    assert abs(ev["rel_err"] - hist[-1]["rel_err"]) <= 1e-6 * hist[-1]["rel_err"]
    nb_train, nb_test = -(-c["ntrain"] // a["batch_size"]), -(-c["ntest"] // a["batch_size"])
    assert len(fused_calls) == a["epochs"] * nb_train             # every training loss went through the kernels
    # the recorder saw the test pass only: the fixture's calls are [3 per train batch ..., 1 per test batch ...] per epoch
    per_epoch = 3 * nb_train + nb_test
    test_idx = [ep * per_epoch + 3 * nb_train + k for ep in range(a["epochs"]) for k in range(nb_test)]
    _check(fx, rec.values(), fx.calls[test_idx], fx.calls_dev[test_idx], hist, model.state_dict(), case)


def test_fit_ns_graphed_is_bit_identical_to_eager():
    """ntrain cut to 4 (batch 4): no short batch, every iteration is a replay of the one captured GraphedTrainStep."""
    from transformerbasednavierstokesolver_amd import data, harness
    case = "ns_up"
    fx = dr.Fixture(case)
    train_full, test_set = dr.ns_datasets(case, DEV)
    train_set = data.ResidentDataset(*[t[:4] for t in train_full.tensors])
    orders = [[i for i in p if i < 4] for p in fx.perms]
    runs = []
    for graphed in (False, True):
        from transformerbasednavierstokesolver_amd.optim import FusedAdamW
        model = _hip_model(case)
        a = dr.parse_argv(dr.CASES[case]["argv"])
        opt = FusedAdamW(model.parameters(), lr=a["lr"], weight_decay=a["weight_decay"])
        sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=a["lr"], epochs=a["epochs"], steps_per_epoch=1)
        from transformerbasednavierstokesolver_amd.utils.testloss import FusedTestLoss
        hist = harness.fit_ns(model, opt, sched, train_set, test_set, epochs=a["epochs"], batch_size=4,
                              loss_fn=FusedTestLoss(size_average=False), epoch_orders=orders, graphed=graphed,
                              grad_sync=opt.sync)
        runs.append((hist, {k: v.detach().clone() for k, v in model.state_dict().items()}))
    (h0, p0), (h1, p1) = runs
    assert h0 == h1, (h0, h1)
    assert all(torch.equal(p0[k], p1[k]) for k in p0), [k for k in p0 if not torch.equal(p0[k], p1[k])]
    assert any(not torch.equal(p0[k].cpu(), torch.from_numpy(dr.weights(case)[k])) for k in p0)     # it did train


def _counted(monkeypatch, module, name):
    hits = []
    real = getattr(module, name)
    monkeypatch.setattr(module, name, lambda *a, **k: (hits.append(1), real(*a, **k))[1])
    return hits


def test_the_fused_switch_keeps_the_exp_ns_loops_off_the_window_kernels(monkeypatch):
    """harness's `fused` switch from both sides, at step = 2 where the two routes differ: 8 x 8 points, C = 32, 4 heads,
    M = 8, 2 layers, out_dim = 2; 3 training and 3 test samples at batch 2 (a short last batch each), T = 4, one epoch.
    fit_ns and evaluate_ns never reach functional.rel_l2_window, ops.rollout_tail or ops.rollout_score; fit_velocity on the
    same data runs every training loss on the first (2 batches x 2 calls) and its test pass on the other two (2 batches x
    2 tails, 2 scores)."""
    import velocity_restatement as vr
    from transformerbasednavierstokesolver_amd import data, functional, harness, ops
    from transformerbasednavierstokesolver_amd.optim import FusedAdamW
    from transformerbasednavierstokesolver_amd.utils.testloss import FusedTestLoss
    train_set, test_set = (data.ResidentDataset(*[t[:3] for t in ds.tensors]) for ds in vr.datasets("velocity", DEV))
    window, tails, scores = (_counted(monkeypatch, functional, "rel_l2_window"), _counted(monkeypatch, ops, "rollout_tail"),
                             _counted(monkeypatch, ops, "rollout_score"))

    def run(fit):
        model = harness.build_model(vr.model_config("velocity"), vr.weights("velocity"), DEV)
        opt = FusedAdamW(model.parameters(), lr=5e-4, weight_decay=1e-5)
        sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=5e-4, epochs=1, steps_per_epoch=2)
        hist = fit(model, opt, sched, train_set, test_set, epochs=1, batch_size=2, T=4, step=2,
                   loss_fn=FusedTestLoss(size_average=False), epoch_orders=[[2, 0, 1]], grad_sync=opt.sync)
        assert len(hist) == 1 and all(np.isfinite(v) and v > 0 for v in hist[0].values()), hist
        return model, hist[0]

    model, last = run(harness.fit_ns)
    ev = harness.evaluate_ns(model, test_set, 2, T=4, step=2, loss_fn=FusedTestLoss(size_average=False))
    # the epoch's test pass again, on the same weights (the bound of the Darcy test above)
    assert sorted(ev) == ["test_full", "test_step"] and all(abs(ev[k] - last[k]) <= 1e-6 * last[k] for k in ev), (ev, last)
    assert (len(window), len(tails), len(scores)) == (0, 0, 0)
    run(harness.fit_velocity)
    assert (len(window), len(tails), len(scores)) == (2 * 2, 2 * 2, 2)


def test_train_command_line_end_to_end(tmp_path):
    """`python -m ...train --driver ns` as a fresh child process on a .mat in a temporary directory; a second child reads
    the checkpoint with --eval 1 and prints the metric of the last epoch's test pass."""
    import scipy.io as scio
    scio.savemat(str(tmp_path / "NavierStokes_V1e-5_N1200_T20.mat"), dr.ns_mat("ns_up"))
    common = [sys.executable, "-m", "transformerbasednavierstokesolver_amd.train", "--driver", "ns", "--data_path", str(tmp_path),
              "--ntrain", "6", "--ntest", "4", "--gpu", "0", "--save_name", "cli"] + dr.CASES["ns_up"]["argv"][:-2]
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = subprocess.run(common, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("Epoch ")]
    assert len(lines) == 2 and os.path.isfile(tmp_path / "checkpoints" / "cli.pt")
    last_full = float(re.search(r"test_full_loss:([0-9.eE+-]+)", lines[-1]).group(1))
    ev = subprocess.run(common + ["--eval", "1"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert ev.returncode == 0, ev.stderr[-2000:]
    shown = float(ev.stdout.strip().splitlines()[-1])
    assert np.isfinite(shown) and abs(shown - last_full) <= 1e-5 + 1e-5 * abs(last_full)
    sd = torch.load(tmp_path / "checkpoints" / "cli.pt", weights_only=True)
    assert set(sd) == set(dr.weights("ns_up"))
