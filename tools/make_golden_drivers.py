"""Golden vectors of the reference's DRIVERS, made by their own main(): tests/golden/G14_exp_ns_epochs.npz,
G15_unrolled_epochs.npz, G16_exp_darcy_epochs.npz.

Runs only where the reference checkout exists (like the other tools/make_golden_*.py; `oracle.make_golden.import_reference()`
installs the import shims).  The drivers (exp_ns.py, ns_vorticity_unrolling.py, exp_darcy.py) only run argparse at import;
their work sits in main().  For every case of tests/driver_restatement.CASES this script

  * sets sys.argv, imports the driver (nn.Module.cuda -> identity, an Agg matplotlib, an empty `phi.torch.flow` stub for the
    unrolled driver) and sets its module globals ntrain / ntest small;
  * patches scipy.io.loadmat to return the seeded synthetic arrays of tests/driver_restatement.py (the fixture keeps seeds
    and sums, not the arrays);
  * wraps the model class the driver builds (model_dict.get_model(...).Model, or SOL_Transolver_Structured_Mesh_2D) so that it
    loads `synth` weights and casts its inputs to the dtype of its parameters;
  * patches RandomSampler.__iter__ to replay the recorded permutations;
  * replaces the module's TestLoss by a recording subclass: every loss value, unrounded, in call order;
  * runs main() in a temporary working directory and reads back the checkpoint it writes;
  * does all of that twice: under default dtype float64 (loadmat then returns float64 arrays of the same values) — the
    EXPECTED values of the fixture — and as written in float32, recorded as the float32 run's OWN DEVIATION per loss call,
    per metric and per parameter tensor (rel-L2).

The unrounded epoch metrics are rebuilt from the loss calls with the drivers' normalisations and checked against the lines
main() printed (5 decimals).  Asserted: at least 90 % of the parameter tensors have own deviation below 1e-5.
Each file also holds the drivers' argparse flags with their defaults, and G16 exp_darcy.central_diff on a seeded 9 x 9 field.

Usage:  python tools/make_golden_drivers.py
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

from oracle.make_golden import GOLD, REF, import_reference  # noqa: E402
import driver_restatement as dr  # noqa: E402

DRIVER_MODULES = {"ns": "exp_ns", "unrolled": "ns_vorticity_unrolling", "darcy": "exp_darcy"}
METRIC_NAMES = {"ns": ["train_step", "train_full", "test_step", "test_full"], "unrolled": ["train_step", "test_step"],
                "darcy": ["reg", "train_loss", "rel_err"]}


def install_shims():
    import_reference()                                   # timm stub, Tensor.cuda -> identity, the reference on sys.path
    torch.nn.Module.cuda = lambda self, *a, **k: self
    import matplotlib
    matplotlib.use("Agg")
    for name in ("phi", "phi.torch", "phi.torch.flow"):
        sys.modules.setdefault(name, types.ModuleType(name))


def import_driver(driver, argv):
    """Import (or re-parse) the driver module with `argv`; its globals derived from args are set again."""
    name = DRIVER_MODULES[driver]
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


def parser_table(mod):
    return [[a.option_strings, a.dest, a.default, getattr(a.type, "__name__", None)]
            for a in mod.parser._actions if a.dest != "help"]


def _load(inner, sd_np):
    res = inner.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def casting_model(cls, sd_np=None):
    """Subclass of the reference Model that casts (x, fx) to the dtype of its parameters (the drivers hand float32
    positions and `.float()` coefficients to a model that the float64 run builds in float64) and, with `sd_np`, loads the
    synth weights after construction."""

    class Casting(cls):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            if sd_np is not None:
                _load(self, sd_np)

        def forward(self, x, fx=None, T=None):
            dt = self.preprocess.linear_post.weight.dtype      # (`placeholder` is float32 whatever the default dtype)
            return super().forward(x.to(dt), None if fx is None else fx.to(dt), T)

    return Casting


def loading_sol(cls, sd_np):
    """Subclass of the reference SOL wrapper that loads the synth weights into its inner Transolver."""

    class Loading(cls):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            _load(self.transolver_model, sd_np)

    return Loading


def run_case(case, dtype):
    """One run of the reference's main().  Returns (loss calls, printed lines, final state_dict, parser table, settings)."""
    c = dr.CASES[case]
    driver = c["driver"]
    mod = import_driver(driver, c["argv"])
    mod.ntrain, mod.ntest = c["ntrain"], c["ntest"]
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    sd_np = dr.weights(case)

    # ---- loadmat -> synthetic arrays
    import scipy.io as scio
    if driver == "darcy":
        tr, te = dr.darcy_mats(case)
        table = {mod.train_path: tr, mod.test_path: te}
        fake = lambda path, *a, **k: {key: v.astype(np_dt) for key, v in table[path].items()}
    else:
        u = dr.ns_mat(case)["u"]
        fake = lambda path, *a, **k: {"u": u.astype(np_dt)}

    # ---- recording TestLoss
    from utils.testloss import TestLoss
    calls = []

    class RecordingTestLoss(TestLoss):
        def __call__(self, x, y):
            v = super().__call__(x, y)
            calls.append(float(v.detach()))
            return v

    # ---- the model class
    import model.Transolver_Structured_Mesh_2D as m2d
    import model.SOL_Transolver_Structured_Mesh_2D as msol
    real_model, real_inner = m2d.Model, msol.transolver_model
    perms = iter(dr.permutations(case))
    real_iter = torch.utils.data.RandomSampler.__iter__
    real_loadmat, real_default = scio.loadmat, torch.get_default_dtype()
    saved = dict(TestLoss=mod.TestLoss)
    out = io.StringIO()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        try:
            torch.set_default_dtype(dtype)
            torch.manual_seed(0)
            scio.loadmat = fake
            mod.scio.loadmat = fake
            mod.TestLoss = RecordingTestLoss
            torch.utils.data.RandomSampler.__iter__ = lambda self: iter(next(perms))
            if driver == "unrolled":
                msol.transolver_model = casting_model(real_inner)          # the class the SOL wrapper instantiates
                saved["SOL"] = mod.SOL_Transolver_Structured_Mesh_2D
                mod.SOL_Transolver_Structured_Mesh_2D = loading_sol(msol.SOL_Transolver_Structured_Mesh_2D, sd_np)
            else:
                # (the reference Model's own super(Model, self) looks `Model` up in its module: that name must stay)
                saved["get_model"] = mod.get_model
                wrapped = types.SimpleNamespace(Model=casting_model(real_model, sd_np))
                mod.get_model = lambda args: wrapped
            os.chdir(tmp)
            with contextlib.redirect_stdout(out):
                mod.main()
            ckpt = torch.load(os.path.join(tmp, "checkpoints", mod.args.save_name + ".pt"), map_location="cpu",
                              weights_only=True)
        finally:
            os.chdir(cwd)
            torch.set_default_dtype(real_default)
            scio.loadmat = real_loadmat
            mod.scio.loadmat = real_loadmat
            mod.TestLoss = saved["TestLoss"]
            torch.utils.data.RandomSampler.__iter__ = real_iter
            m2d.Model, msol.transolver_model = real_model, real_inner
            if "SOL" in saved:
                mod.SOL_Transolver_Structured_Mesh_2D = saved["SOL"]
            if "get_model" in saved:
                mod.get_model = saved["get_model"]
    final = {k: v.double().numpy() for k, v in ckpt.items()}
    assert all(v.dtype == dtype for k, v in ckpt.items() if k != "placeholder"), "the run did not happen in the requested dtype"
    return np.array(calls, dtype=np.float64), out.getvalue().splitlines(), final, parser_table(mod), vars(mod.args).copy()


def metrics_from_calls(case, calls):
    """The drivers' unrounded epoch metrics from the loss calls ([epochs, k]); consumes every call."""
    c, a = dr.CASES[case], dr.parse_argv(dr.CASES[case]["argv"])
    ntrain, ntest, bs, epochs = c["ntrain"], c["ntest"], a["batch_size"], a["epochs"]
    nb_train, nb_test = -(-ntrain // bs), -(-ntest // bs)
    it = iter(calls.tolist())
    take = lambda n: sum(next(it) for _ in range(n))
    rows = []
    if c["driver"] == "ns":
        for _ in range(epochs):
            ts = tf = es = ef = 0.0
            for _ in range(nb_train):
                ts += take(dr.T)
                tf += take(1)
            for _ in range(nb_test):
                es += take(dr.T)
                ef += take(1)
            rows.append([ts / ntrain / dr.T, tf / ntrain, es / ntest / dr.T, ef / ntest])
    elif c["driver"] == "unrolled":
        la, thresh = 1, epochs / 2
        for ep in range(epochs):
            if ep % thresh == 0 and ep >= thresh and la <= 10:
                la = min(la * 2, 10)
                thresh /= 2
            ts = sum(take(len(range(0, dr.T - la + 1, la))) for _ in range(nb_train))
            es = sum(take(dr.T) for _ in range(nb_test))
            rows.append([ts, es / ntest / dr.T])
    else:
        for _ in range(epochs):
            l2 = reg = 0.0
            for _ in range(nb_train):
                l2 += take(1)
                reg += take(2)
            err = sum(take(1) for _ in range(nb_test))
            rows.append([reg / ntrain, l2 / ntrain, err / ntest])
    assert next(it, None) is None, "loss calls left over: the call structure is not what this script assumes"
    return np.array(rows)


def printed_metrics(case, lines):
    """The numbers main() printed per epoch, in METRIC_NAMES order."""
    driver = dr.CASES[case]["driver"]
    num = r"([-+0-9.eE]+|nan|inf)"
    rows = []
    if driver == "ns":
        for ln in lines:
            m = re.match(rf"Epoch \d+ , train_step_loss:{num} , train_full_loss:{num} , test_step_loss:{num} , test_full_loss:{num}", ln)
            if m:
                rows.append([float(g) for g in m.groups()])
    elif driver == "unrolled":
        tr = [float(m.group(1)) for ln in lines if (m := re.match(rf"Epoch \d+ , train_step_loss:{num}", ln))]
        te = [float(m.group(1)) for ln in lines if (m := re.match(rf"Epoch \d+ , test_step_loss:{num}", ln))]
        rows = [list(p) for p in zip(tr, te)]
    else:
        tr = [(float(m.group(1)), float(m.group(2))) for ln in lines
              if (m := re.match(rf"Epoch \d+ Reg : {num} Train loss : {num}", ln))]
        te = [float(m.group(1)) for ln in lines if (m := re.match(rf"rel_err:{num}", ln))]
        rows = [[a, b, e] for (a, b), e in zip(tr, te)]
    return np.array(rows)


def make_case(case, out):
    c = dr.CASES[case]
    calls64, lines64, final64, table, args = run_case(case, torch.float64)
    calls32, lines32, final32, _, _ = run_case(case, torch.float32)
    assert calls64.shape == calls32.shape and np.all(np.isfinite(calls64)) and np.all(np.isfinite(calls32))
    met64, met32 = metrics_from_calls(case, calls64), metrics_from_calls(case, calls32)
    for met, lines in ((met64, lines64), (met32, lines32)):      # the decomposition reproduces what main() printed
        shown = printed_metrics(case, lines)
        assert shown.shape == met.shape, (case, shown.shape, met.shape)
        assert np.all(np.abs(shown - met) <= 6e-6 + 1e-6 * np.abs(met)), (case, shown, met)
    pdev = {k: float(np.linalg.norm((final32[k] - v).ravel()) / max(np.linalg.norm(v.ravel()), 1e-300))
            for k, v in final64.items()}
    moved = [k for k, v in final64.items() if not np.array_equal(v, dr.weights(case)[k].astype(np.float64))]
    tight = sum(d < 1e-5 for d in pdev.values()) / len(pdev)
    print(f"  {case}: {calls64.size} loss calls, own deviation: calls max {np.abs(calls32 - calls64).max():.2e}, params max "
          f"{max(pdev.values()):.2e} median {np.median(list(pdev.values())):.2e} ({tight:.0%} below 1e-5), "
          f"{len(moved)} of {len(final64)} tensors moved")
    assert tight >= 0.9, f"{case}: only {tight:.0%} of the parameter tensors have own deviation below 1e-5: shorten the case"
    assert len(moved) >= len(final64) - 1, "training moved too few tensors (only `placeholder` may stay)"
    pre = case + "."
    settings = dict(argv=c["argv"], args=args, driver=c["driver"], ntrain=c["ntrain"], ntest=c["ntest"], T_in=dr.T_IN, T=dr.T,
                    step=1, weight_seed=c["weight_seed"], data_seed=c["data_seed"], data_sums=dr.data_sums(case),
                    metric_names=METRIC_NAMES[c["driver"]], config=dr.model_config(case),
                    scheduler_epochs=dr.DARCY_SCHEDULER_EPOCHS if c["driver"] == "darcy" else args["epochs"])
    out[pre + "settings"] = np.array(json.dumps(settings))
    out[pre + "printed"] = np.array(json.dumps([ln for ln in lines64 if ln.startswith(("Epoch", "rel_err"))]))
    out[pre + "perms"] = np.array(dr.permutations(case), dtype=np.int64)
    out[pre + "calls"], out[pre + "calls_dev"] = calls64, np.abs(calls32 - calls64)
    out[pre + "metrics"], out[pre + "metrics_dev"] = met64, np.abs(met32 - met64)
    out[pre + "params_dev"] = np.array(json.dumps(pdev))
    for k, v in final64.items():
        out[pre + "param." + k] = v
    return c["driver"], table


def main():
    if not os.path.isdir(REF):
        sys.exit(f"{REF} not found: this generator runs only next to the reference checkout")
    install_shims()
    files = {}
    for case, c in dr.CASES.items():
        out = files.setdefault(c["file"], {})
        driver, table = make_case(case, out)
        out["parser." + driver] = np.array(json.dumps(table))
    # exp_darcy.central_diff on a seeded 9 x 9 field (float64)
    darcy = import_driver("darcy", dr.CASES["darcy"]["argv"])
    f = dr.central_diff_field()
    gx, gy = darcy.central_diff(torch.from_numpy(f).double(), 1.0 / dr.CENTRAL_DIFF_RES, dr.CENTRAL_DIFF_RES)
    g16 = files["G16_exp_darcy_epochs.npz"]
    g16["central_diff.field_sum"] = np.asarray(np.sum(f, dtype=np.float64))
    g16["central_diff.gx"], g16["central_diff.gy"] = gx.numpy(), gy.numpy()
    for name, out in files.items():
        path = os.path.join(GOLD, name)
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        print("wrote", path, size, "bytes")
        assert size < 1_000_000, f"{name}: {size} bytes, keep it under 1 MB"


if __name__ == "__main__":
    main()
