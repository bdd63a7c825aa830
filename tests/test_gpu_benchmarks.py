"""The airfoil / pipe / elasticity / plasticity epoch loops on the HIP path against the reference scripts' own main()
(fixtures G17-G20): the HIP models (default engine) with optim.FusedAdamW and FusedTestLoss through harness.fit_static (x 3)
and harness.fit_plas.  Bounds, as tests/test_gpu_drivers.py: max(floor, 4 x the fixture's own deviation) with 1e-5 on loss
calls and metrics, 1e-5 rel-L2 on final parameters (2e-3 for to_q / to_k).  Spies: every training loss of a run went
through the decoded rel-L2 kernels (functional.rel_l2_affine) and every model call through the embedding kernel
(ops.embed_bias_fwd).  Then `--driver pipe` end to end in a fresh child process, and `--eval 1` on its checkpoint."""
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
LOSS_FLOOR, PARAM_FLOOR, QK_FLOOR = 1e-5, 1e-5, 2e-3


def _hip_model(case):
    from transformerbasednavierstokesolver_amd import harness
    from transformerbasednavierstokesolver_amd.model import Transolver_Irregular_Mesh
    cfg, sd = br.model_config(case), br.weights(case)
    if case != "elas":
        return harness.build_model(cfg, sd, DEV)
    m = Transolver_Irregular_Mesh.Model(space_dim=2, n_layers=cfg["n_layers"], n_hidden=cfg["n_hidden"], dropout=0.0,
                                        n_head=cfg["n_head"], Time_Input=False, mlp_ratio=cfg["mlp_ratio"], fun_dim=0,
                                        out_dim=1, slice_num=cfg["slice_num"], ref=cfg["ref"], unified_pos=cfg["unified_pos"])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.to(DEV)


def _fused_adamw(model, case):
    from transformerbasednavierstokesolver_amd.optim import FusedAdamW
    a = br.parse_argv(br.CASES[case]["argv"])
    opt = FusedAdamW(model.parameters(), lr=a["lr"], weight_decay=a["weight_decay"], max_grad_norm=a["max_grad_norm"])
    return a, opt, br.scheduler(opt, case)


def _recorder():
    """FusedTestLoss that keeps every value it returns, in call order (device tensors: no synchronisation in the loop)."""
    from transformerbasednavierstokesolver_amd.utils.testloss import FusedTestLoss

    class Recording(FusedTestLoss):
        def __init__(self):
            super().__init__(size_average=False)
            self.log = []

        def rel_decoded(self, pred, y, normalizer=None):
            v = FusedTestLoss.rel_decoded(self, pred, y, normalizer)
            self.log.append(v.detach())
            return v

        def __call__(self, x, y):
            v = FusedTestLoss.rel(self, x, y)
            self.log.append(v.detach())
            return v

        def values(self):
            return np.array([float(v) for v in self.log], dtype=np.float64)

    return Recording()


class Spies:
    """Counts model calls (forward pre-hook), fused loss calls (functional.rel_l2_affine, with the target it was handed)
    and embedding kernel calls (ops.embed_bias_fwd, with which addends)."""

    def __init__(self, monkeypatch, model):
        from transformerbasednavierstokesolver_amd import functional, ops
        self.model_calls, self.train_calls, self.loss_targets, self.embeds = 0, 0, [], []
        real_loss, real_embed = functional.rel_l2_affine, ops.embed_bias_fwd

        def loss(pred, y, mean=None, std=None):
            self.loss_targets.append((y, mean is not None))
            return real_loss(pred, y, mean, std)

        def embed(h, placeholder=None, tvec=None, out=None):
            self.embeds.append((placeholder is not None, tvec is not None))
            return real_embed(h, placeholder, tvec, out)

        def count(module, args):
            self.model_calls += 1
            self.train_calls += int(module.training)

        monkeypatch.setattr(functional, "rel_l2_affine", loss)
        monkeypatch.setattr(ops, "embed_bias_fwd", embed)
        model.register_forward_pre_hook(count)


def _check(case, fx, rec, history, state_dict):
    dr.check_scalars(rec.values(), fx.calls, fx.calls_dev, LOSS_FLOOR, case + " loss calls")
    dr.check_scalars(br.script_metrics(case, history), fx.metrics, fx.metrics_dev, LOSS_FLOOR, case + " metrics")
    worst = dr.check_params(state_dict, fx, PARAM_FLOOR, QK_FLOOR, label=case)
    print(case, "worst parameter rel-L2:", max(worst.items(), key=lambda kv: kv[1]))


@pytest.mark.parametrize("case", ["airfoil", "pipe", "elas"])
def test_fit_static_on_the_hip_path(case, monkeypatch):
    from transformerbasednavierstokesolver_amd import harness
    fx = br.Fixture(case)
    model = _hip_model(case)
    a, opt, sched = _fused_adamw(model, case)
    spies = Spies(monkeypatch, model)
    rec = _recorder()
    d = br.load_data(case)
    hist = harness.fit_static(model, opt, sched, d, epochs=a["epochs"], batch_size=a["batch_size"], loss_fn=rec,
                              epoch_orders=fx.perms, scheduler_per_epoch=case == "elas", grad_sync=opt.sync)
    _check(case, fx, rec, hist, model.state_dict())
    train_idx = br.train_call_indices(case)
    assert spies.train_calls == len(train_idx) and spies.model_calls == fx.calls.size
    # every training loss went through the decoded rel-L2 kernels, with the normaliser where the script decodes
    assert len(spies.loss_targets) == len(train_idx)
    assert all(has_norm == (case != "airfoil") for _, has_norm in spies.loss_targets)
    # every model call (training and test) embedded through the kernel: fx = None, so the placeholder alone
    assert spies.embeds == [(True, False)] * spies.model_calls
    if d["y_normalizer"] is not None:
        assert d["y_normalizer"].mean.device.type == "cpu"            # the caller's normaliser stays where it was
    ev = harness.evaluate_static(model, d, a["batch_size"], _recorder())
    assert abs(ev["rel_err"] - hist[-1]["rel_err"]) <= 1e-6 * hist[-1]["rel_err"]


def test_fit_plas_on_the_hip_path(monkeypatch):
    from transformerbasednavierstokesolver_amd import harness
    case = "plas"
    fx = br.Fixture(case)
    model = _hip_model(case)
    a, opt, sched = _fused_adamw(model, case)
    spies = Spies(monkeypatch, model)
    rec = _recorder()
    d = br.load_data(case)
    hist = harness.fit_plas(model, opt, sched, d, epochs=a["epochs"], batch_size=a["batch_size"], loss_fn=rec,
                            epoch_orders=fx.perms, time_orders=fx.time_perms, grad_sync=opt.sync)
    _check(case, fx, rec, hist, model.state_dict())
    train_idx = br.train_call_indices(case)
    nb_test = -(-br.PLAS_LIMIT["test"] // a["batch_size"])
    steps = len(train_idx) + a["epochs"] * nb_test * br.PLAS_T            # one model call per step loss, training and test
    assert spies.train_calls == len(train_idx) and spies.model_calls == steps and opt.steps == len(train_idx)
    # every step loss went through the kernels on the [B, N, 4, 1] time slice itself: element stride T, no reshape copy
    assert len(spies.loss_targets) == steps
    assert all(not has_norm and y.shape[-1] == 1 and y.stride(2) == br.PLAS_T for y, has_norm in spies.loss_targets)
    # fx is given (no placeholder) and T is: every model call added its time vector through the kernel
    assert spies.embeds == [(False, True)] * steps
    ev = harness.evaluate_plas(model, d, a["batch_size"], _recorder())
    assert abs(ev["test_full"] - hist[-1]["test_full"]) <= 1e-6 * hist[-1]["test_full"]


def test_train_command_line_end_to_end_pipe(tmp_path):
    """`python -m ...train --driver pipe` as a fresh child process on Pipe_{X,Y,Q}.npy in a temporary directory (30 samples
    of the 129 x 129 mesh, strided to 9 x 9); a second child reads the checkpoint with --eval 1 and prints the metric of
    the last epoch's test pass."""
    from transformerbasednavierstokesolver_amd import synth
    X, Y, Q = synth.mesh_field_arrays(30, 129, 129, channels=2, channel=0, seed=5)
    for name, arr in (("X", X), ("Y", Y), ("Q", Q)):
        np.save(str(tmp_path / f"Pipe_{name}.npy"), arr)
    common = [sys.executable, "-m", "transformerbasednavierstokesolver_amd.train", "--driver", "pipe", "--data_path", str(tmp_path),
              "--ntrain", "20", "--ntest", "6", "--gpu", "0", "--save_name", "cli_pipe", "--batch-size", "8", "--epochs", "2",
              "--downsamplex", "16", "--downsampley", "16"] + br.MODEL_2D
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = subprocess.run(common, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert len([ln for ln in lines if re.match(r"Epoch \d+ Train loss : \d+\.\d{5}$", ln)]) == 2
    errs = [float(ln.split(":", 1)[1]) for ln in lines if ln.startswith("rel_err:")]
    assert len(errs) == 2 and os.path.isfile(tmp_path / "checkpoints" / "cli_pipe.pt")
    ev = subprocess.run(common + ["--eval", "1"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert ev.returncode == 0, ev.stderr[-2000:]
    last = ev.stdout.strip().splitlines()[-1]
    assert last.startswith("rel_err:")
    shown = float(last.split(":", 1)[1])
    assert np.isfinite(shown) and abs(shown - errs[-1]) <= 1e-5 + 1e-5 * abs(errs[-1])
    sd = torch.load(tmp_path / "checkpoints" / "cli_pipe.pt", weights_only=True)
    assert set(sd) == set(br.weights("pipe"))
