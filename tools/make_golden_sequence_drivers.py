"""Golden vectors of the latent-sequence DRIVERS, made by their own loops: tests/golden/G21_auto_encoder_epochs.npz
(auto_encoder.main()) and G22_sequensolver_merged_epochs.npz (SequenSolverMerged.train()).

Runs only where the reference checkout exists, on the CPU, with the shims of tools/make_golden_drivers.py and
tools/make_golden_sequensolver_merged.py and nothing else of the reference's code:

  * auto_encoder.py runs argparse at import: sys.argv is set, the module globals ntrain / ntest are set small, and
    model_dict.get_model(...).Model is wrapped so that it loads `synth` weights and casts its inputs to its parameters' dtype;
  * SequenSolverMerged.train() reads the module global `args` (set here to 2 epochs, sim_num = 2), builds its model from a
    hard-coded encoder checkpoint (the name `SequenSolver` it calls is replaced by a function that builds the seeded model
    with the arguments train() passes) and hard-codes 10 test samples: the SECOND TensorDataset it builds (the test set) is limited to TEST_LIMIT samples, as PLAS_LIMIT does in
    make_golden_benchmarks.py; the metrics keep the script's divisor ntest = 10.  The model is the one
    make_golden_sequensolver_merged.build() makes (seeded weights, `temperature` a plain tensor at 0.5);
  * scipy.io.loadmat returns a seeded synthetic `u` (the fixture keeps the seed and the sum, not the array);
  * RandomSampler.__iter__ replays recorded permutations; the module's TestLoss is a recording subclass (every loss value,
    unrounded, in call order), from which the unrounded epoch metrics are rebuilt with the scripts' own divisors and checked
    against the printed lines where the script prints rounded ones;
  * everything runs twice: under default dtype float64 (the EXPECTED values) and as written in float32, whose deviation
    from the float64 run is stored as `fp32_self_error.<key>`.

Per file: settings (JSON), the permutations, metrics [epochs, k], per parameter after training `param.<key>` (whole if small,
else norm and a strided sample), `fp32_self_error.*`, and `bound.*` = max(4 x fp32_self_error, base) with base 1e-5 for the
metrics (losses) and 1e-4 for the parameters.  Asserted: at least 90 % of the trained parameter tensors have own
deviation below 1e-5.

Usage:  python tools/make_golden_sequence_drivers.py
"""
from __future__ import annotations

import argparse
import contextlib
import importlib
import io
import json
import os
import sys
import tempfile
import types

os.environ.setdefault("MPLBACKEND", "Agg")

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.make_golden import GOLD, REF, import_reference  # noqa: E402
from make_golden_3d import put  # noqa: E402
from make_golden_sequensolver import _Float64Numpy  # noqa: E402
import make_golden_sequensolver_merged as g13  # noqa: E402
from sequence_driver_restatement import permutations, synthetic_u  # noqa: E402
from transformerbasednavierstokesolver_amd import synth  # noqa: E402

BASE = {"metrics": 1e-5, "param": 1e-4}
T = 10
AE = dict(argv=["--model", "Transolver_Structured_Mesh2D_Encoder", "--n-hidden", "16", "--n-layers", "2", "--n-heads", "1",
                "--slice_num", "8", "--batch-size", "8", "--epochs", "2", "--lr", "0.001", "--save_name", "g21"],
          ntrain=2, ntest=1, weight_seed=211, data_seed=212, perm_seed=213, epochs=2, batch_size=8)
SEQ = dict(epochs=2, sim_num=2, ntest=10, test_limit=1, seed=221, data_seed=222, perm_seed=223, trajectories=12,
           layers=8, sequential_head=16, save_name="g22")


class _Patches(contextlib.ExitStack):
    def set(self, obj, name, value):
        if hasattr(obj, name):
            self.callback(setattr, obj, name, getattr(obj, name))
        else:                   # e.g. SequenSolverMerged.args, which only its __main__ creates
            self.callback(delattr, obj, name)
        setattr(obj, name, value)


def _recording(TestLoss, calls):
    class RecordingTestLoss(TestLoss):
        def __call__(self, x, y):
            v = super().__call__(x, y)
            calls.append(float(v.detach()))
            return v
    return RecordingTestLoss


def _run(mod, entry, dtype, u, perms, ckpt_name, extra):
    """entry() under the common patches; returns (loss calls, printed lines, checkpoint as float64 numpy)."""
    import scipy.io as scio
    from utils.testloss import TestLoss
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    calls, out, it = [], io.StringIO(), iter(perms)
    cwd, real_default = os.getcwd(), torch.get_default_dtype()
    with tempfile.TemporaryDirectory() as tmp, _Patches() as p:
        p.callback(os.chdir, cwd)
        p.callback(torch.set_default_dtype, real_default)
        torch.set_default_dtype(dtype)
        torch.manual_seed(0)
        fake = lambda path, *a, **k: {"u": u.astype(np_dt)}
        p.set(scio, "loadmat", fake)
        p.set(mod, "TestLoss", _recording(TestLoss, calls))
        p.set(torch.utils.data.RandomSampler, "__iter__", lambda self: iter(next(it)))
        os.chdir(tmp)
        extra(p, tmp)
        with contextlib.redirect_stdout(out):
            entry()
        ckpt = torch.load(os.path.join(tmp, "sequential_checkpoints", ckpt_name + ".pt"), map_location="cpu", weights_only=True)
    return np.array(calls, dtype=np.float64), out.getvalue().splitlines(), {k: v.double().numpy() for k, v in ckpt.items()}


# ---------------------------------------------------------------------------------------------- auto_encoder.main()
def run_auto_encoder(dtype):
    old = sys.argv
    sys.argv = ["auto_encoder.py"] + AE["argv"]
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            mod = importlib.import_module("auto_encoder")
        mod.args = mod.parser.parse_args(AE["argv"])
    finally:
        sys.argv = old
    mod.eval, mod.save_name = mod.args.eval, mod.args.save_name
    mod.ntrain, mod.ntest = AE["ntrain"], AE["ntest"]
    import model.Transolver_Structured_Mesh2D_Encoder as enc
    spec_holder = {}

    class Casting(enc.Model):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            spec = [(key, tuple(v.shape)) for key, v in self.state_dict().items()]
            sd = synth.synth_state_dict_from_spec(spec, seed=AE["weight_seed"])
            res = self.load_state_dict({key: torch.from_numpy(v).to(self.state_dict()[key].dtype) for key, v in sd.items()},
                                       strict=True)
            assert not res.missing_keys and not res.unexpected_keys
            spec_holder["spec"], spec_holder["sd"] = spec, sd

        def forward(self, x, fx=None, T=None):
            dt = self.preprocess.linear_post.weight.dtype
            return super().forward(x.to(dt), None if fx is None else fx.to(dt), T)

    def extra(p, tmp):
        p.set(mod, "get_model", lambda args: types.SimpleNamespace(Model=Casting))

    u = synthetic_u(AE["data_seed"], AE["ntrain"] + AE["ntest"])
    perms = permutations(AE["perm_seed"], AE["epochs"], AE["ntrain"] * 20)
    calls, lines, final = _run(mod, mod.main, dtype, u, perms, "g21", extra)
    nb_train, nb_test = -(-AE["ntrain"] * 20 // AE["batch_size"]), -(-AE["ntest"] * 20 // AE["batch_size"])
    assert calls.size == AE["epochs"] * (nb_train + nb_test), "the call structure is not what this script assumes"
    per = calls.reshape(AE["epochs"], nb_train + nb_test)
    metrics = np.stack([per[:, :nb_train].sum(1) / AE["ntrain"] / (T / 1), per[:, nb_train:].sum(1) / AE["ntest"] / (T / 1)], 1)
    shown = [ln for ln in lines if ln.startswith("Epoch")]
    for ep, ln in enumerate(shown):      # the script prints the unrounded metrics
        assert f"train_step_loss:{metrics[ep, 0]}" in ln and f"test_step_loss:{metrics[ep, 1]}" in ln, (ln, metrics[ep])
    assert len(shown) == AE["epochs"]
    return metrics, final, perms, spec_holder, u


# ---------------------------------------------------------------------------------------------- SequenSolverMerged.train()
def run_merged(mod, dtype):
    cfg = dict(B=1, T=T, layers=SEQ["layers"], sequential_head=SEQ["sequential_head"], seed=SEQ["seed"])
    real_cls, holder = mod.SequenSolver, {}

    def make(path, **kw):       # train() calls SequenSolver(transolver_path, T=..., ..., layers=8, sequential_head=16)
        assert (kw["layers"], kw["sequential_head"], kw["B"], kw["T"]) == (cfg["layers"], cfg["sequential_head"], 1, T)
        mod.SequenSolver = real_cls
        try:
            m, spec, sd = g13.build(mod, cfg, dtype)
        finally:
            mod.SequenSolver = make
        holder["spec"], holder["sd"] = spec, sd
        return m

    count = [0]
    real_ds = torch.utils.data.TensorDataset

    def limited(*tensors):      # 1st: the train set; 2nd: the test set, cut to TEST_LIMIT samples
        count[0] += 1
        if count[0] == 2:
            tensors = tuple(t[:SEQ["test_limit"]] for t in tensors)
        return real_ds(*tensors)

    def extra(p, tmp):
        p.set(mod, "SequenSolver", make)
        p.set(mod, "np", _Float64Numpy() if dtype == torch.float64 else np)
        p.set(torch.utils.data, "TensorDataset", limited)
        p.set(mod, "args", argparse.Namespace(eval=0, epochs=SEQ["epochs"], save_name=SEQ["save_name"], sim_num=SEQ["sim_num"]))

    u = synthetic_u(SEQ["data_seed"], SEQ["trajectories"])
    perms = permutations(SEQ["perm_seed"], SEQ["epochs"], SEQ["sim_num"])
    calls, lines, final = _run(mod, lambda: mod.train(eval=False), dtype, u, perms, SEQ["save_name"], extra)
    per_train, per_test = T + 1, T + 2                 # step terms + full; step terms + first frame + full
    n_ep = SEQ["sim_num"] * per_train + SEQ["test_limit"] * per_test
    assert calls.size == SEQ["epochs"] * n_ep, "the call structure is not what this script assumes"
    rows = []
    for ep in range(SEQ["epochs"]):
        c = calls[ep * n_ep:(ep + 1) * n_ep]
        tr = c[:SEQ["sim_num"] * per_train].reshape(SEQ["sim_num"], per_train)
        te = c[SEQ["sim_num"] * per_train:].reshape(SEQ["test_limit"], per_test)
        rows.append([tr[:, :T].sum() / SEQ["sim_num"] / T, tr[:, T].sum() / SEQ["sim_num"], te[:, :T].sum() / SEQ["ntest"] / T,
                     te[:, T + 1].sum() / SEQ["ntest"], te[:, T].sum() / SEQ["ntest"]])
    metrics = np.array(rows)
    shown = [ln for ln in lines if ln.startswith("Epoch")]
    assert len(shown) == SEQ["epochs"]
    for ep, ln in enumerate(shown):      # printed with 5 decimals
        want = "train_step_loss:{:.5f} , train_full_loss:{:.5f} , test_step_loss:{:.5f} , test_full_loss:{:.5f}".format(*metrics[ep, :4])
        assert want in ln, (ln, want)
    return metrics, final, perms, holder, u


def store(out, metrics64, metrics32, final64, final32, start_sd, perms, settings, holder, u, metric_names):
    pdev = {k: float(np.linalg.norm((final32[k] - v).ravel()) / max(np.linalg.norm(v.ravel()), 1e-300)) for k, v in final64.items()}
    moved = [k for k, v in final64.items() if k in start_sd and not np.array_equal(v, start_sd[k].astype(np.float64))]
    tight = sum(pdev[k] < 1e-5 for k in moved) / len(moved)
    mdev = np.abs(metrics32 - metrics64) / np.abs(metrics64)
    print(f"  metrics own deviation max {mdev.max():.2e}; {len(moved)} of {len(final64)} tensors moved, own deviation max "
          f"{max(pdev[k] for k in moved):.2e}, {tight:.0%} below 1e-5")
    assert tight >= 0.9, f"only {tight:.0%} of the trained tensors have own deviation below 1e-5: choose another size"
    spec = holder["spec"]
    out["settings"] = np.array(json.dumps(dict(settings, metric_names=metric_names, base=BASE, moved=moved)))
    out["keys"] = np.array([k for k, _ in spec])
    out["shapes"] = np.array(json.dumps([list(s) for _, s in spec]))
    out["sums"] = np.array([np.sum(holder["sd"][k], dtype=np.float64) for k, _ in spec])
    out["data_sum"] = np.asarray(np.sum(u, dtype=np.float64))
    out["perms"] = np.array(perms, dtype=np.int64)
    out["metrics"] = metrics64
    out["fp32_self_error.metrics"] = mdev
    out["bound.metrics"] = np.maximum(4 * mdev, BASE["metrics"])
    for k in moved:
        put(out, "param." + k, final64[k])
        out["fp32_self_error.param." + k] = np.asarray(pdev[k])
        out["bound.param." + k] = np.asarray(max(4 * pdev[k], BASE["param"]))


def main():
    if not os.path.isdir(REF):
        sys.exit(f"{REF} not found: this generator runs only next to the reference checkout")
    import_reference()
    torch.nn.Module.cuda = lambda self, *a, **k: self
    real_ones = torch.ones
    torch.ones = lambda *a, device=None, **k: real_ones(*a, **k)      # the merged constructor's mask asks for device='cuda'
    import matplotlib.pyplot as plt
    plt.show = lambda *a, **k: None
    files = {}

    print("auto_encoder.main()")
    m64, f64, perms, holder, u = run_auto_encoder(torch.float64)
    m32, f32, _, _, _ = run_auto_encoder(torch.float32)
    out = files.setdefault("G21_auto_encoder_epochs.npz", {})
    store(out, m64, m32, f64, f32, holder["sd"], perms, {k: v for k, v in AE.items()}, holder, u, ["train_step", "test_step"])

    print("SequenSolverMerged.train()")
    import SequenSolverMerged as mod
    m64, f64, perms, holder, u = run_merged(mod, torch.float64)
    m32, f32, _, _, _ = run_merged(mod, torch.float32)
    out = files.setdefault("G22_sequensolver_merged_epochs.npz", {})
    settings = dict(SEQ, geometry=g13.GEOM, slice_scale=g13.SLICE_SCALE, lr=1e-3, weight_decay=1e-5, Tin=T, Tout=T)
    store(out, m64, m32, f64, f32, holder["sd"], perms, settings, holder, u,
          ["train_step", "train_full", "test_step", "test_full", "test_first"])

    for name, out in files.items():
        path = os.path.join(GOLD, name)
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        print("wrote", path, size, "bytes")
        assert size <= 1_000_000, f"{name}: {size} bytes, keep it at or under 1 MB"


if __name__ == "__main__":
    main()
