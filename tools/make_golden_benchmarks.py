"""Golden vectors of the reference's remaining benchmark DRIVERS, made by their own main(): tests/golden/
G17_exp_airfoil_epochs.npz, G18_exp_pipe_epochs.npz, G19_exp_elas_epochs.npz, G20_exp_plas_epochs.npz.

Runs only where the reference checkout exists.  The shims, the casting model, the recorded sampler permutations, the
recording TestLoss and the two runs (float64: the EXPECTED values; float32 as written: the reference's OWN DEVIATION) are
those of tools/make_golden_drivers.py.  For every case of tests/benchmark_restatement.CASES this script

  * imports the driver with the case's argv (exp_plas imports numpy / torch after its argparse: nothing to shim there);
  * patches np.load / scipy.io.loadmat to return the seeded synthetic arrays of tests/benchmark_restatement.py, picked by
    file name;
  * exp_airfoil / exp_pipe keep their hard-coded 1000 / 200 samples: the meshes are shrunk by the scripts' own downsample
    flags and --batch-size 400 keeps an epoch at three steps;
  * exp_elas.py:102 reads an undefined global `epochs` (the script raises as shipped): the module global is set to
    --epochs, which is what this project's driver passes to CosineAnnealingLR;
  * exp_plas hard-codes 101 x 31, T = 20 and 900 / 80 samples as locals of main(): torch.utils.data.TensorDataset is wrapped
    so that the loaders see only the first PLAS_LIMIT samples of each split, torch.randperm replays the recorded time
    permutations of random_collate_fn, and the timestep embedding (which the script computes in float32 whatever the
    model's dtype) is cast to the model's dtype in the float64 run;
  * the model class is wrapped to load `synth` weights and cast its inputs; in the float64 run `placeholder` (created as
    float32 by the reference whatever the default dtype) is made float64 too, so that EXPECTED is float64 throughout.

The unrounded epoch metrics are rebuilt from the loss calls with the scripts' own divisors and checked against the lines
main() printed.  Asserted: at least 90 % of the parameter tensors have own deviation below 1e-5.

Usage:  python tools/make_golden_benchmarks.py
"""
from __future__ import annotations

import contextlib
import importlib
import io
import json
import os
import re
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle.make_golden import GOLD, REF  # noqa: E402
import benchmark_restatement as br  # noqa: E402
import make_golden_drivers as mgd  # noqa: E402

DRIVER_MODULES = {"airfoil": "exp_airfoil", "pipe": "exp_pipe", "elas": "exp_elas", "plas": "exp_plas"}


def import_driver(case, argv):
    name = DRIVER_MODULES[case]
    old = sys.argv
    sys.argv = [name + ".py"] + list(argv)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            mod = importlib.import_module(name)
        mod.args = mod.parser.parse_args(argv)
    finally:
        sys.argv = old
    mod.eval, mod.save_name = mod.args.eval, mod.args.save_name
    return mod


def casting_model(cls, sd_np):
    """mgd.casting_model, plus: `placeholder` and the unified-position grid follow the default dtype."""
    base = mgd.casting_model(cls, sd_np)

    class Casting(base):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.placeholder.data = self.placeholder.data.to(torch.get_default_dtype())
            if getattr(self, "unified_pos", 0) and torch.is_tensor(getattr(self, "pos", None)):
                self.pos = self.pos.to(torch.get_default_dtype())     # without fx nothing promotes the float32 grid

    return Casting


class LimitedTensorDataset(torch.utils.data.TensorDataset):
    """TensorDataset of the first `limit` samples; the limits are handed out in construction order (train, test)."""
    limits = []

    def __init__(self, *tensors):
        n = LimitedTensorDataset.limits.pop(0)
        super().__init__(*[t[:n] for t in tensors])


def run_case(case, dtype):
    c = br.CASES[case]
    mod = import_driver(case, c["argv"])
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    sd_np = br.weights(case)
    arrays = br.file_arrays(case)
    if case == "elas":
        mod.epochs = mod.args.epochs
    import scipy.io as scio
    from utils.testloss import TestLoss
    calls = []

    class RecordingTestLoss(TestLoss):
        def __call__(self, x, y):
            v = super().__call__(x, y)
            calls.append(float(v.detach()))
            return v

    module_name = "model.Transolver_Irregular_Mesh" if case == "elas" else "model.Transolver_Structured_Mesh_2D"
    mmod = importlib.import_module(module_name)
    wrapped = types.SimpleNamespace(Model=casting_model(mmod.Model, sd_np))
    perms = iter(br.permutations(case))
    tperms = iter([p for ep in br.time_permutations() for p in ep]) if case == "plas" else None
    real = dict(iter=torch.utils.data.RandomSampler.__iter__, np_load=np.load, loadmat=scio.loadmat,
                default=torch.get_default_dtype(), TestLoss=mod.TestLoss, get_model=mod.get_model,
                randperm=torch.randperm, TensorDataset=torch.utils.data.TensorDataset,
                embedding=getattr(mmod, "timestep_embedding", None))
    out = io.StringIO()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        try:
            torch.set_default_dtype(dtype)
            torch.manual_seed(0)
            np.load = lambda path, *a, **k: arrays[os.path.basename(path)].astype(np_dt)
            scio.loadmat = lambda path, *a, **k: {key: v.astype(np_dt) for key, v in arrays.items()}
            mod.TestLoss = RecordingTestLoss
            mod.get_model = lambda args: wrapped
            torch.utils.data.RandomSampler.__iter__ = lambda self: iter(next(perms))
            if case == "plas":
                LimitedTensorDataset.limits = [br.PLAS_LIMIT["train"], br.PLAS_LIMIT["test"]]
                torch.utils.data.TensorDataset = LimitedTensorDataset
                torch.randperm = lambda n, *a, **k: torch.tensor(next(tperms), dtype=torch.long)
                mmod.timestep_embedding = lambda *a, **k: real["embedding"](*a, **k).to(torch.get_default_dtype())
            os.chdir(tmp)
            with contextlib.redirect_stdout(out):
                mod.main()
            ckpt = torch.load(os.path.join(tmp, "checkpoints", mod.args.save_name + ".pt"), map_location="cpu",
                              weights_only=True)
        finally:
            os.chdir(cwd)
            torch.set_default_dtype(real["default"])
            np.load, scio.loadmat = real["np_load"], real["loadmat"]
            mod.TestLoss, mod.get_model = real["TestLoss"], real["get_model"]
            torch.utils.data.RandomSampler.__iter__ = real["iter"]
            torch.randperm, torch.utils.data.TensorDataset = real["randperm"], real["TensorDataset"]
            if real["embedding"] is not None:
                mmod.timestep_embedding = real["embedding"]
    assert next(perms, None) is None and (tperms is None or next(tperms, None) is None), "permutations left over"
    final = {k: v.double().numpy() for k, v in ckpt.items()}
    assert all(v.dtype == dtype for v in ckpt.values()), "the run did not happen in the requested dtype"
    return np.array(calls, dtype=np.float64), out.getvalue().splitlines(), final, mgd.parser_table(mod), vars(mod.args).copy()


def metrics_from_calls(case, calls):
    """The scripts' unrounded epoch metrics from the loss calls, with THEIR divisors; consumes every call."""
    c, a = br.CASES[case], br.parse_argv(br.CASES[case]["argv"])
    ntrain, ntest, bs = c["ntrain"], c["ntest"], a["batch_size"]
    nb_train, nb_test = -(-br.seen_train(case) // bs), -(-br.seen_test(case) // bs)
    it = iter(calls.tolist())
    take = lambda n: sum(next(it) for _ in range(n))
    rows = []
    for _ in range(a["epochs"]):
        if case == "plas":
            T = br.PLAS_T
            tr = take(nb_train * T)
            step = full = 0.0
            for _ in range(nb_test):
                step += take(T)
                full += take(1)
            rows.append([tr / ntrain / T, step / ntest / T, full / ntest])
        else:
            rows.append([take(nb_train) / ntrain, take(nb_test) / ntest])
    assert next(it, None) is None, "loss calls left over: the call structure is not what this script assumes"
    return np.array(rows)


def printed_metrics(case, lines):
    num = r"([-+0-9.eE]+|nan|inf)"
    if case == "plas":
        pat = rf"Epoch \d+ , train_step_loss:{num} , test_step_loss:{num} , test_full_loss:{num}"
        return np.array([[float(g) for g in m.groups()] for ln in lines if (m := re.match(pat, ln))])
    tr = [float(m.group(1)) for ln in lines if (m := re.match(rf"Epoch \d+ Train loss : {num}", ln))]
    te = [float(m.group(1)) for ln in lines if (m := re.match(rf"rel_err ?: ?{num}", ln))]
    return np.array([list(p) for p in zip(tr, te)])


def make_case(case):
    c = br.CASES[case]
    calls64, lines64, final64, table, args = run_case(case, torch.float64)
    calls32, lines32, final32, _, _ = run_case(case, torch.float32)
    assert calls64.shape == calls32.shape and np.all(np.isfinite(calls64)) and np.all(np.isfinite(calls32))
    met64, met32 = metrics_from_calls(case, calls64), metrics_from_calls(case, calls32)
    for met, lines in ((met64, lines64), (met32, lines32)):
        shown = printed_metrics(case, lines)
        assert shown.shape == met.shape, (case, shown.shape, met.shape)
        # the train / step metrics are printed with 5 decimals, rel_err unrounded
        assert np.all(np.abs(shown - met) <= 6e-6 + 1e-6 * np.abs(met)), (case, shown, met)
    pdev = {k: float(np.linalg.norm((final32[k] - v).ravel()) / max(np.linalg.norm(v.ravel()), 1e-300))
            for k, v in final64.items()}
    start = br.weights(case)
    moved = [k for k, v in final64.items() if not np.array_equal(v, start[k].astype(np.float64))]
    tight = sum(d < 1e-5 for d in pdev.values()) / len(pdev)
    print(f"  {case}: {calls64.size} loss calls, own deviation: calls max {np.abs(calls32 - calls64).max():.2e}, params max "
          f"{max(pdev.values()):.2e} median {np.median(list(pdev.values())):.2e} ({tight:.0%} below 1e-5), "
          f"{len(moved)} of {len(final64)} tensors moved")
    assert tight >= 0.9, f"{case}: only {tight:.0%} of the parameter tensors have own deviation below 1e-5: shorten the case"
    assert len(moved) >= len(final64) - 1, "training moved too few tensors (only `placeholder` may stay)"
    pre = case + "."
    settings = dict(argv=c["argv"], args=args, driver=c["driver"], ntrain=c["ntrain"], ntest=c["ntest"],
                    seen_train=br.seen_train(case), seen_test=br.seen_test(case), weight_seed=c["weight_seed"],
                    data_seed=c["data_seed"], data_sums=br.data_sums(case), metric_names=br.METRIC_NAMES[case],
                    config=br.model_config(case))
    out = {pre + "settings": np.array(json.dumps(settings)),
           pre + "printed": np.array(json.dumps([ln for ln in lines64 if ln.startswith(("Epoch", "rel_err"))])),
           pre + "perms": np.array(br.permutations(case), dtype=np.int64),
           pre + "calls": calls64, pre + "calls_dev": np.abs(calls32 - calls64),
           pre + "metrics": met64, pre + "metrics_dev": np.abs(met32 - met64),
           pre + "params_dev": np.array(json.dumps(pdev)), "parser." + case: np.array(json.dumps(table))}
    if case == "plas":
        out[pre + "time_perms"] = np.array(br.time_permutations(), dtype=np.int64)
    for k, v in final64.items():
        out[pre + "param." + k] = v
    return out


def main():
    if not os.path.isdir(REF):
        sys.exit(f"{REF} not found: this generator runs only next to the reference checkout")
    mgd.install_shims()
    for case, c in br.CASES.items():
        out = make_case(case)
        path = os.path.join(GOLD, c["file"])
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        print("wrote", path, size, "bytes")
        assert size < 1_000_000, f"{c['file']}: {size} bytes, keep it under 1 MB"


if __name__ == "__main__":
    main()
