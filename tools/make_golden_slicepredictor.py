"""Golden vectors of the conv slice predictors: tests/golden/G12_slicepredictor.npz.

Runs only where the reference checkout exists, on the CPU (like tools/make_golden_learnslice.py;
`oracle.make_golden.import_reference()` installs the import shims).  It imports the reference's top-level SliceLearner.py
(class SliceLearner) and LearnSlice.py (class LearnSlice; the trainers behind `__main__` do not run) and records:

  keys.slicelearner.default / .small   [[key, shape], ...] of the reference's SliceLearner state_dict (JSON): default
                                       constructor, and the small configuration of tests/slicepredictor_restatement.SMALL
  keys.learnslice.code / .nocode       the same for the predictor part (preprocess, in_project_x, in_project_slice,
                                       temperature) of LearnSlice(1, 1, use_code_for_vorticity=True / False).  Under the shims
                                       `.cuda()` is the identity, so `temperature` stays a registered Parameter; on a GPU the
                                       reference loses it (`nn.Parameter(...).cuda()` is a plain tensor)
  signature.slicelearner               parameters and defaults of SliceLearner.__init__ (JSON)
  small.*                              SliceLearner at the small shape (6 x 5 mesh, n_hidden 32, M 12, B 2): sw.f64 / sw.f32
                                       [2, 1, 30, 12], grad.<key> (float64) of sum(sw * dsw) for every parameter the forward
                                       reads, state_sum / input_sums (x, fx, dsw)
  vort.<case>.*                        LearnSlice.forward_from_vorticity at the reference's fixed shape (N = 4096, 74 features,
                                       n_hidden 256, M 16, C 32, B 1), case `code` (with the code) and `nocode`: sw.f64 / .f32
                                       at every 7th point with sw.norm.*, sw.max (the largest weight), loss.f64 / .f32 =
                                       F.mse_loss(sw, target), grad.<key>.norm and grad.<key>.sample (every k-th element,
                                       float64) of the loss for every predictor parameter, state_sum / input_sums

Weights and inputs are NOT stored (the 256 x 256 x 3 x 3 conv weight alone is 2.4 MB): tests/slicepredictor_restatement.py owns
the seeded numpy generator that draws them, for this tool and for the tests, and both sides check them by their sums.  The
last layer is scaled up so that some points have a largest weight above 0.9 (asserted here): the default-initialised
reference gives weights in 0.016-0.20, which hides errors.

Usage:  python tools/make_golden_slicepredictor.py
"""
from __future__ import annotations

import inspect
import json
import os
import sys

os.environ["MPLBACKEND"] = "Agg"

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))      # slicepredictor_restatement: one generator for both sides

from oracle.make_golden import GOLD, REF, import_reference, rel  # noqa: E402
import slicepredictor_restatement as R  # noqa: E402

PREDICTOR = ("preprocess.", "in_project_x.", "in_project_slice.")


def keys_json(sd, only=None):
    return np.array(json.dumps([[k, list(v.shape)] for k, v in sd.items() if only is None or k.startswith(only)]))


def load(m, sd, dtype):
    res = m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not res.unexpected_keys, res.unexpected_keys
    return m.to(dtype)


def run_small(SL, out):
    sd, x, fx, dsw = R.small_case()
    out["small.state_sum"] = np.asarray(R.state_sum(sd))
    out["small.input_sums"] = R.input_sums((x, fx, dsw))
    res = {}
    for dtype in (torch.float64, torch.float32):
        m = SL(**R.SMALL)
        missing = m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        assert not missing.missing_keys and not missing.unexpected_keys
        m = m.to(dtype)
        sw = m(torch.from_numpy(x).to(dtype), torch.from_numpy(fx).to(dtype))
        assert sw.dtype == dtype and sw.shape == (R.SMALL_B, 1, 30, 12)
        res[dtype] = sw.detach()
        if dtype == torch.float64:
            (sw * torch.from_numpy(dsw).double()).sum().backward()
            for k, p in m.named_parameters():
                if p.grad is not None:
                    out[f"small.grad.{k}"] = p.grad.numpy().astype(np.float64)
    out["small.sw.f64"] = res[torch.float64].numpy().astype(np.float64)
    out["small.sw.f32"] = res[torch.float32].numpy().astype(np.float32)
    big = float(res[torch.float64].max())
    print(f"  small: fp32 self error {rel(res[torch.float32], res[torch.float64]):.2e}, largest weight {big:.3f}")
    assert big > 0.9


def run_vort(LS, name, out):
    cfg = R.VORT_CASES[name]
    sd, x, fx, code, target = R.vort_case(name)
    key = f"vort.{name}"
    out[key + ".state_sum"] = np.asarray(R.state_sum(sd))
    out[key + ".input_sums"] = R.input_sums([a for a in (x, fx, code, target) if a is not None])
    res = {}
    for dtype in (torch.float64, torch.float32):
        m = load(LS(unified_pos=1, use_vorticity=1, use_code_for_vorticity=cfg["use_code"]), sd, dtype)
        if dtype == torch.float64:
            out[f"keys.learnslice.{name}"] = np.array(json.dumps(
                [[k, list(v.shape)] for k, v in m.state_dict().items() if k == "temperature" or k.startswith(PREDICTOR)]))
            assert [k for k, _ in json.loads(str(out[f"keys.learnslice.{name}"]))] == list(sd), "generator key order"
        c = None if code is None else torch.from_numpy(code).to(dtype)
        sw = m.forward_from_vorticity(torch.from_numpy(x).to(dtype), torch.from_numpy(fx).to(dtype), c)
        assert sw.dtype == dtype and sw.shape == (1, 1, 4096, 16)
        loss = F.mse_loss(sw, torch.from_numpy(target).to(dtype))
        res[dtype] = (sw.detach(), float(loss.detach()))
        if dtype == torch.float64:
            loss.backward()
            grads = dict(m.named_parameters())
            for k in sd:
                n, s = R.grad_sample(grads[k].grad.numpy())
                out[f"{key}.grad.{k}.norm"] = np.asarray(n)
                out[f"{key}.grad.{k}.sample"] = s
    for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
        a = res[dt][0].double().numpy()[0, 0]
        out[f"{key}.sw.{tag}"] = a[::R.STRIDE].astype(np.float64 if tag == "f64" else np.float32)
        out[f"{key}.sw.norm.{tag}"] = np.asarray(np.linalg.norm(a))
        out[f"{key}.loss.{tag}"] = np.asarray(res[dt][1])
    big = res[torch.float64][0].max(-1).values
    out[key + ".sw.max"] = np.asarray(float(big.max()))
    print(f"  {name}: fp32 self error {rel(res[torch.float32][0], res[torch.float64][0]):.2e}, loss {res[torch.float64][1]:.6g}, "
          f"largest weight {float(big.max()):.3f}, {int((big > 0.9).sum())} points above 0.9")
    assert int((big > 0.9).sum()) > 0


def main():
    if not os.path.isdir(REF):
        sys.exit(f"{REF} not found: this generator runs only next to the reference checkout")
    import_reference()
    import matplotlib.pyplot as plt
    plt.show = lambda *a, **k: None
    import SliceLearner as sl_mod
    import LearnSlice as ls_mod
    SL, LS = sl_mod.SliceLearner, ls_mod.LearnSlice
    out = {}
    out["signature.slicelearner"] = np.array(json.dumps(
        [[k, None if p.default is inspect.Parameter.empty else p.default]
         for k, p in inspect.signature(SL.__init__).parameters.items() if k != "self"]))
    out["keys.slicelearner.default"] = keys_json(SL().state_dict())
    out["keys.slicelearner.small"] = keys_json(SL(**R.SMALL).state_dict())
    shp = R.slice_learner_shapes(**{k: v for k, v in R.SMALL.items() if k not in ("H", "W")})
    assert R.key_list(out, "keys.slicelearner.small") == shp, "the restatement's shape list is the reference's"
    print("SliceLearner, small case")
    run_small(SL, out)
    for name in R.VORT_CASES:
        print(f"forward_from_vorticity, case {name}")
        run_vort(LS, name, out)
    path = os.path.join(GOLD, "G12_slicepredictor.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size <= 1_000_000, "the fixture must stay at or under 1 MB"


if __name__ == "__main__":
    main()
