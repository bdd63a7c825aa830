"""Golden vectors of the reference's velocity-field DRIVERS, made by their own main(): tests/golden/G25_ns_velocity_epochs.npz,
G26_velocity_unrolled_epochs.npz, G27_unrolled_t_epochs.npz.

In the manner of tools/make_golden_drivers.py, whose shims and wrappers this script reuses; it runs only where the reference
checkout exists.  ns_velocity.py, ns_velocity_unrolling.py and ns_unrolling2_with_t.py only run argparse at import; their
work sits in main().  For every case of tests/velocity_restatement.CASES this script

  * sets sys.argv, imports the script (nn.Module.cuda -> identity, an empty `phi.torch.flow` stub) and sets its module
    globals ntrain / ntest small; T_in, T, step and max_look_ahead stay the script's own;
  * patches numpy.load to return the seeded synthetic array of tests/velocity_restatement.py (the fixture keeps seeds and
    sums, not the array);
  * wraps the model class the script builds so that it loads `synth` weights and casts its inputs to its parameters' dtype;
  * patches RandomSampler.__iter__ to replay the recorded permutations;
  * replaces the module's TestLoss by a recording subclass: every loss value, unrounded, in call order;
  * runs main() in a temporary working directory and reads back the checkpoint it writes;
  * does all of that twice: under default dtype float64 (numpy.load then returns a float64 array of the same values), the
    EXPECTED values of the fixture, and as written in float32, recorded as the float32 run's OWN DEVIATION per loss call,
    per metric and per parameter tensor (rel-L2).

The runs are long enough for the look-ahead curriculum to move (42 epochs: 1 -> 2; 22 epochs: 1 -> 2 -> 3).  The unrounded
epoch metrics are rebuilt from the loss calls with the scripts' normalisations and checked against the lines main()
printed (5 decimals).  Asserted: at least 90 % of the parameter tensors have own deviation below 1e-5.  Each file also holds
the script's argparse flags with their defaults and its module constants.

Usage:  python tools/make_golden_velocity_drivers.py
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
import make_golden_drivers as base  # noqa: E402
import velocity_restatement as vr  # noqa: E402

CONSTANTS = ("ntrain", "ntest", "T_in", "T", "step", "LOOK_AHEAD", "max_look_ahead")
_shipped = {}       # module name -> its constants at first import (a later run sees the small ntrain / ntest)


def import_script(case, argv):
    name = vr.script(case)["module"]
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


def run_case(case, dtype):
    """One run of the script's main().  Returns (loss calls, printed lines, final state_dict, parser table, args, constants)."""
    c = vr.CASES[case]
    mod = import_script(case, c["argv"])
    constants = _shipped.setdefault(mod.__name__, {k: getattr(mod, k) for k in CONSTANTS if hasattr(mod, k)})
    s = vr.script(case)
    assert all(constants[k] == s[k] for k in ("ntrain", "ntest", "T_in", "T")) and constants["step"] == vr.STEP, constants
    assert constants.get("max_look_ahead") == s["max_look_ahead"], constants
    mod.ntrain, mod.ntest = c["ntrain"], c["ntest"]
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    sd_np = vr.weights(case)
    arr = vr.array(case)
    fake = lambda path, *a, **k: arr.astype(np_dt)

    from utils.testloss import TestLoss
    calls = []

    class RecordingTestLoss(TestLoss):
        def __call__(self, x, y):
            v = super().__call__(x, y)
            calls.append(float(v.detach()))
            return v

    import model.Transolver_Structured_Mesh_2D as m2d
    import model.SOL_Transolver_Structured_Mesh_2D as msol
    real_model, real_inner = m2d.Model, msol.transolver_model
    perms = iter(vr.permutations(case))
    real_iter = torch.utils.data.RandomSampler.__iter__
    real_load, real_default = np.load, torch.get_default_dtype()
    saved = dict(TestLoss=mod.TestLoss)
    out = io.StringIO()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        try:
            torch.set_default_dtype(dtype)
            torch.manual_seed(0)
            np.load = fake
            mod.TestLoss = RecordingTestLoss
            torch.utils.data.RandomSampler.__iter__ = lambda self: iter(next(perms))
            if c["driver"] == "velocity":
                saved["get_model"] = mod.get_model
                wrapped = types.SimpleNamespace(Model=base.casting_model(real_model, sd_np))
                mod.get_model = lambda args: wrapped
            else:
                msol.transolver_model = base.casting_model(real_inner)          # the class the SOL wrapper instantiates
                saved["SOL"] = mod.SOL_Transolver_Structured_Mesh_2D
                mod.SOL_Transolver_Structured_Mesh_2D = base.loading_sol(msol.SOL_Transolver_Structured_Mesh_2D, sd_np)
            os.chdir(tmp)
            with contextlib.redirect_stdout(out):
                mod.main()
            np.load = real_load
            ckpt = torch.load(os.path.join(tmp, "checkpoints", mod.args.save_name + ".pt"), map_location="cpu",
                              weights_only=True)
        finally:
            os.chdir(cwd)
            torch.set_default_dtype(real_default)
            np.load = real_load
            mod.TestLoss = saved["TestLoss"]
            torch.utils.data.RandomSampler.__iter__ = real_iter
            m2d.Model, msol.transolver_model = real_model, real_inner
            if "SOL" in saved:
                mod.SOL_Transolver_Structured_Mesh_2D = saved["SOL"]
            if "get_model" in saved:
                mod.get_model = saved["get_model"]
    final = {k: v.double().numpy() for k, v in ckpt.items()}
    assert all(v.dtype == dtype for k, v in ckpt.items() if k != "placeholder"), "the run did not happen in the requested dtype"
    return (np.array(calls, dtype=np.float64), out.getvalue().splitlines(), final, base.parser_table(mod), vars(mod.args).copy(),
            constants)


def metrics_from_calls(case, calls):
    """The scripts' unrounded epoch metrics from the loss calls ([epochs, k]); consumes every call."""
    c, a, s = vr.CASES[case], vr.parse_argv(vr.CASES[case]["argv"]), vr.script(case)
    ntrain, ntest, bs = c["ntrain"], c["ntest"], a["batch_size"]
    nb_train, nb_test, S = -(-ntrain // bs), -(-ntest // bs), s["T"] // vr.STEP
    it = iter(calls.tolist())
    take = lambda n: sum(next(it) for _ in range(n))
    rows = []
    for la in vr.look_ahead_history(case):
        if c["driver"] == "velocity":
            ts = tf = es = ef = 0.0
            for _ in range(nb_train):
                ts += take(S)
                tf += take(1)
            for _ in range(nb_test):
                es += take(S)
                ef += take(1)
            rows.append([ts / ntrain / S, tf / ntrain, es / ntest / S, ef / ntest])
            continue
        ts = sum(take(vr.train_calls(case, la)) for _ in range(nb_train))
        es = sum(take(S) for _ in range(nb_test))
        rows.append([es / ntest / S] if c["driver"] == "velocity_unrolled" else [ts, es / ntest / S])
    assert next(it, None) is None, "loss calls left over: the call structure is not what this script assumes"
    return np.array(rows)


def printed_metrics(case, lines):
    """The numbers main() printed per epoch, in METRIC_NAMES order."""
    driver = vr.CASES[case]["driver"]
    num = r"([-+0-9.eE]+|nan|inf)"
    if driver == "velocity":
        pat = rf"Epoch \d+ , train_step_loss:{num} , train_full_loss:{num} , test_step_loss:{num} , test_full_loss:{num}"
        return np.array([[float(g) for g in m.groups()] for ln in lines if (m := re.match(pat, ln))])
    te = [float(m.group(1)) for ln in lines if (m := re.match(rf"Epoch \d+ , test_step_loss:{num}", ln))]
    if driver == "velocity_unrolled":
        return np.array([[v] for v in te])
    tr = [float(m.group(1)) for ln in lines if (m := re.match(rf"Epoch \d+ , train_step_loss:{num}", ln))]
    return np.array([list(p) for p in zip(tr, te)])


def make_case(case, out):
    c = vr.CASES[case]
    calls64, lines64, final64, table, args, constants = run_case(case, torch.float64)
    calls32, lines32, final32, _, _, _ = run_case(case, torch.float32)
    assert calls64.shape == calls32.shape and np.all(np.isfinite(calls64)) and np.all(np.isfinite(calls32))
    met64, met32 = metrics_from_calls(case, calls64), metrics_from_calls(case, calls32)
    for met, lines in ((met64, lines64), (met32, lines32)):      # the decomposition reproduces what main() printed
        shown = printed_metrics(case, lines)
        assert shown.shape == met.shape, (case, shown.shape, met.shape)
        assert np.all(np.abs(shown - met) <= 6e-6 + 1e-6 * np.abs(met)), (case, shown, met)
    history = vr.look_ahead_history(case)
    raised = [int(m.group(1)) for ln in lines64 if (m := re.match(r"look ahead increased (\d+)", ln))]
    assert raised == sorted(set(history) - {1}), (case, raised, history)
    if case in vr.LOOK_AHEAD_HISTORY:
        assert history == vr.LOOK_AHEAD_HISTORY[case]
    pdev = {k: float(np.linalg.norm((final32[k] - v).ravel()) / max(np.linalg.norm(v.ravel()), 1e-300))
            for k, v in final64.items()}
    moved = [k for k, v in final64.items() if not np.array_equal(v, vr.weights(case)[k].astype(np.float64))]
    tight = sum(d < 1e-5 for d in pdev.values()) / len(pdev)
    print(f"  {case}: {calls64.size} loss calls, own deviation: calls max {np.abs(calls32 - calls64).max():.2e}, params max "
          f"{max(pdev.values()):.2e} median {np.median(list(pdev.values())):.2e} ({tight:.0%} below 1e-5), "
          f"{len(moved)} of {len(final64)} tensors moved")
    assert tight >= 0.9, f"{case}: only {tight:.0%} of the parameter tensors have own deviation below 1e-5: shorten the case"
    assert len(moved) >= len(final64) - 1, "training moved too few tensors (only `placeholder` may stay)"
    pre = case + "."
    s = vr.script(case)
    settings = dict(argv=c["argv"], args=args, driver=c["driver"], ntrain=c["ntrain"], ntest=c["ntest"], T_in=s["T_in"], T=s["T"],
                    step=vr.STEP, constants=constants, look_ahead=history, weight_seed=c["weight_seed"],
                    data_seed=c["data_seed"], data_sums=vr.data_sums(case), metric_names=vr.METRIC_NAMES[c["driver"]],
                    config=vr.model_config(case), scheduler_epochs=args["epochs"])
    out[pre + "settings"] = np.array(json.dumps(settings))
    out[pre + "printed"] = np.array(json.dumps([ln for ln in lines64 if ln.startswith(("Epoch", "look ahead"))]))
    out[pre + "perms"] = np.array(vr.permutations(case), dtype=np.int64)
    out[pre + "calls"], out[pre + "calls_dev"] = calls64, np.abs(calls32 - calls64)
    out[pre + "metrics"], out[pre + "metrics_dev"] = met64, np.abs(met32 - met64)
    out[pre + "params_dev"] = np.array(json.dumps(pdev))
    for k, v in final64.items():
        out[pre + "param." + k] = v
    return c["driver"], table


def main():
    if not os.path.isdir(REF):
        sys.exit(f"{REF} not found: this generator runs only next to the reference checkout")
    base.install_shims()
    files = {}
    for case, c in vr.CASES.items():
        out = files.setdefault(c["file"], {})
        driver, table = make_case(case, out)
        out["parser." + driver] = np.array(json.dumps(table))
    for name, out in files.items():
        path = os.path.join(GOLD, name)
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        print("wrote", path, size, "bytes")
        assert size < 1_000_000, f"{name}: {size} bytes, keep it under 1 MB"


if __name__ == "__main__":
    main()
