"""The epoch loops of the latent-sequence family against fixtures that the reference's OWN loops made
(tools/make_golden_sequence_drivers.py): tests/golden/G21_auto_encoder_epochs.npz by auto_encoder.main() and
G22_sequensolver_merged_epochs.npz by SequenSolverMerged.train(), each run in float64 (the expected values) and in float32
(the reference's own deviation, `fp32_self_error.*`).

`harness.fit_autoencoder` and `harness.fit_sequensolver(fold_time=False and True)` run on the same seeded data, weights and
sample orders.  Every epoch metric and every trained parameter tensor is held to the bound the fixture stores:
max(4 x fp32_self_error, base), base 1e-5 for the metrics (losses) and 1e-4 for the parameters.  The merged
script hard-codes ntest = 10 as the divisor of its test metrics; the fixture's test set is its first sample alone, so the
loop's metrics (divided by the samples it saw) are rescaled by 1 / 10 before they are compared.  Every figure is printed
before it is asserted."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import sequence_driver_restatement as SD
import sequensolver_merged_restatement as RM
import sequensolver_restatement as RP

pytestmark = pytest.mark.gpu
G21 = os.path.join(GOLDEN, "G21_auto_encoder_epochs.npz")
G22 = os.path.join(GOLDEN, "G22_sequensolver_merged_epochs.npz")


def _spec(g):
    return list(zip([str(k) for k in g["keys"]], json.loads(str(g["shapes"]))))


def _checked(g, sd, u):
    sums = np.array([np.sum(sd[k], dtype=np.float64) for k, _ in _spec(g)])
    np.testing.assert_allclose(sums, g["sums"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(np.sum(u, dtype=np.float64), float(g["data_sum"]), rtol=1e-12)


def _judge(g, hist, model, scale, label):
    s = json.loads(str(g["settings"]))
    got = np.array([[h[k] for k in s["metric_names"]] for h in hist]) * np.asarray(scale)
    want, bound = g["metrics"], g["bound.metrics"]
    err = np.abs(got - want) / np.abs(want)
    for ep in range(len(hist)):
        for j, k in enumerate(s["metric_names"]):
            print(f"{label} epoch {ep} {k}: {got[ep, j]:.9g} against {want[ep, j]:.9g}, rel {err[ep, j]:.3g}, bound {bound[ep, j]:.3g}")
    assert np.all(bound >= s["base"]["metrics"]) and np.all(err <= bound), (label, err, bound)
    params, worst = dict(model.named_parameters()), (0.0, None)
    assert s["moved"], label
    for k in s["moved"]:
        e, b = RP.golden_rel(g, "param." + k, params[k]), float(g["bound.param." + k])
        assert b >= s["base"]["param"]
        worst = max(worst, (e / b, k))
        assert e <= b, (label, k, e, b)
    print(f"{label}: {len(s['moved'])} trained tensors, worst error / bound {worst[0]:.3g} ({worst[1]})")


def test_fit_autoencoder_against_the_scripts_own_epochs():
    from transformerbasednavierstokesolver_amd import data, harness, synth
    from transformerbasednavierstokesolver_amd.model import Transolver_Structured_Mesh2D_Encoder
    from transformerbasednavierstokesolver_amd.optim import FusedAdamW
    g = np.load(G21)
    s = json.loads(str(g["settings"]))
    u = SD.synthetic_u(s["data_seed"], s["ntrain"] + s["ntest"])
    sd = synth.synth_state_dict_from_spec(_spec(g), seed=s["weight_seed"])
    _checked(g, sd, u)
    model = Transolver_Structured_Mesh2D_Encoder.Model(space_dim=2, n_layers=2, n_hidden=16, dropout=0.0, n_head=1,
                                                       Time_Input=False, mlp_ratio=1, fun_dim=1, out_dim=1, slice_num=8, ref=8,
                                                       unified_pos=0, H=64, W=64)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model = model.cuda()
    d = data.split_ns_all_frames(u, s["ntrain"], s["ntest"])
    steps = -(-s["ntrain"] * 20 // s["batch_size"])
    opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-5)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-3, epochs=s["epochs"], steps_per_epoch=steps)
    perms = g["perms"].tolist()
    assert perms == SD.permutations(s["perm_seed"], s["epochs"], s["ntrain"] * 20)
    hist = harness.fit_autoencoder(model, opt, sched, d, epochs=s["epochs"], batch_size=s["batch_size"], ntrain=s["ntrain"],
                                   ntest=s["ntest"], epoch_orders=perms, grad_sync=opt.sync)
    _judge(g, hist, model, 1.0, "G21 fit_autoencoder")


@pytest.mark.parametrize("fold", [False, True])
def test_fit_sequensolver_merged_against_the_scripts_own_epochs(fold):
    from transformerbasednavierstokesolver_amd import data, harness
    from transformerbasednavierstokesolver_amd.SequenSolverMerged import SequenSolver
    from transformerbasednavierstokesolver_amd.optim import FusedAdamW
    g = np.load(G22)
    s = json.loads(str(g["settings"]))
    u = SD.synthetic_u(s["data_seed"], s["trajectories"])
    sd = RM.draw_state(_spec(g), s["seed"], s["slice_scale"])
    _checked(g, sd, u)
    sd = {k: torch.from_numpy(v) for k, v in sd.items()}
    enc = {k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}
    model = SequenSolver(enc, T=s["Tin"], B=1, layers=s["layers"], sequential_head=s["sequential_head"], **s["geometry"])
    model.load_state_dict(sd, strict=True)
    model = model.cuda()
    split = data.split_ns_trajectories(u, s["sim_num"], s["ntest"], s["Tin"], s["Tout"])
    train = data.ResidentDataset(split["train_a"], split["train_u"], device="cuda")
    test = data.ResidentDataset(split["test_a"][:s["test_limit"]], split["test_u"][:s["test_limit"]], device="cuda")
    opt = FusedAdamW(model.parameters(), lr=s["lr"], weight_decay=s["weight_decay"])
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=s["lr"], epochs=s["epochs"], steps_per_epoch=s["sim_num"])
    perms = g["perms"].tolist()
    assert perms == SD.permutations(s["perm_seed"], s["epochs"], s["sim_num"])
    hist = harness.fit_sequensolver(model, opt, sched, data.unified_positions(64, 64), train, test, epochs=s["epochs"],
                                    variant="merged", fold_time=fold, epoch_orders=perms, grad_sync=opt.sync)
    # the script divides its test sums by its hard-coded ntest = 10; the loop divided by the samples it saw
    k = s["test_limit"] / s["ntest"]
    _judge(g, hist, model, [1.0, 1.0, k, k, k], f"G22 fit_sequensolver fold_time={fold}")
