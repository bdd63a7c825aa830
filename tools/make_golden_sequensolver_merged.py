"""Golden vectors of the merged SequenSolver: tests/golden/G13_sequensolver_merged.npz.

Runs only where the reference checkout exists, on the CPU (conventions of tools/make_golden_sequensolver.py;
`oracle.make_golden.import_reference()` installs the import shims).  It imports the reference's top-level
SequenSolverMerged.py (class SequenSolver; the training behind `__main__` does not run) and runs it at the reference's only
shape (64 x 64, M=16, C=32, T=10, 64 positional features, the hard-coded encoder) in two cases on float32-representable
weights and inputs: `a` (B=2, layers=2, sequential_head=4: seq_dim 128, the unfused attention route) and `b` (B=1, layers=8,
sequential_head=16: the configuration of the reference's __main__, seq_dim 32, the fused route).

Two shims beyond import_reference(), in this process only: `torch.ones` drops `device` (the constructor builds its mask
with device='cuda'), and `temperature` is taken out of the module's parameters and left as a plain tensor at 0.5: on a GPU
`nn.Parameter(...).cuda()` is a plain tensor, in no state_dict and no optimizer, while the `.cuda()` identity shim would
register it.

  weights   tests/sequensolver_merged_restatement.draw_state (synth.synth_state_dict_from_spec by key and shape), the three
            weight matrices of in_project_slice times SLICE_SCALE so that the mean largest predicted slice weight per
            point lies in [0.3, 0.9] (asserted; default initialisation gives 0.10 against the uniform 1/16, which pins
            little).  The encoder's part goes through a temporary file as `transolver_path`.  The fixture keeps keys,
            shapes, seed, scale and sums.
  inputs    pos [B, N, 64]: the unified_pos distances formed in float64 and rounded once; fx, y, yy: seeded standard
            normals; all checked by their sums.
  <case>.pred.*     forward(use_gt=False): out, code, slice weights (strided sample, norm, total sum), the loss
                    TestLoss(size_average=False)(out, y), every parameter gradient, the parameters without one.
  <case>.frozen.*   after freeze_attention(): the frozen names, loss and gradients.
  <case>.get_code   get_code(pos, fx, y): no positional encoding.
  a.gt.out          forward(use_gt=True): the same output (asserted equal to a.pred.out bit for bit in the reference).
  a.train.losses    three iterations of the reference's training loop (use_gt=False, the window slides on with the true
                    frame): AdamW(1e-3, weight_decay 1e-5), OneCycleLR(max_lr 1e-3, epochs=10, steps_per_epoch=10), Tout=2.
  a.rollout.*       its evaluation loop, two steps with the prediction fed back (use_gt=False): pred, step loss, full loss.
  signature         the constructor's parameters and defaults (JSON).

The float64 run replaces the name `np` that the reference module sees by a proxy whose float32 is numpy's float64 (the
reference allocates its token buffer as float32 numpy); the positional table stays the reference's fp32 one.
`fp32_self_error.<key>` holds the rel-L2 between the reference's float32 and float64 results per quantity.

Usage:  python tools/make_golden_sequensolver_merged.py
"""
from __future__ import annotations

import inspect
import json
import os
import sys
import tempfile

os.environ.setdefault("MPLBACKEND", "Agg")

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))      # sequensolver_merged_restatement: one generator for both sides

from oracle.make_golden import GOLD, REF, import_reference, rel  # noqa: E402
from make_golden_3d import put  # noqa: E402
from make_golden_sequensolver import BOUNDS, _Float64Numpy, bound_of, zero  # noqa: E402,F401
import sequensolver_merged_restatement as R  # noqa: E402

GEOM = dict(H=64, W=64, M=16, C=32)
CASES = {"a": dict(B=2, T=10, layers=2, sequential_head=4, seed=61),
         "b": dict(B=1, T=10, layers=8, sequential_head=16, seed=62)}
SLICE_SCALE = {"linear_pre.0.weight": 1.5, "linears.0.0.weight": 1.5, "linear_post.weight": 2.0}
TRAIN = dict(steps=3, lr=1e-3, weight_decay=1e-5, epochs=10, steps_per_epoch=10, Tout=2)


def plain_temperature(m):
    """What the reference is on a GPU: `temperature` a plain tensor at 0.5, outside parameters and state_dict."""
    if "temperature" in m._parameters:
        del m._parameters["temperature"]
    m.temperature = torch.ones([1, 1, 1, 1]) * 0.5
    return m


def build(mod, cfg, dtype):
    torch.manual_seed(cfg["seed"])
    kw = dict(T=cfg["T"], H=GEOM["H"], W=GEOM["W"], M=GEOM["M"], C=GEOM["C"], B=cfg["B"], layers=cfg["layers"],
              sequential_head=cfg["sequential_head"])
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "encoder.pt")
        torch.save({}, path)                                # keys / shapes first: the constructor wants a file
        m = plain_temperature(mod.SequenSolver(path, **kw))
        spec = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
        sd = R.draw_state(spec, cfg["seed"], SLICE_SCALE)
        torch.save({k[len("encoder."):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith("encoder.")}, path)
        m = plain_temperature(mod.SequenSolver(path, **kw))
    own = {k: torch.from_numpy(v) for k, v in sd.items() if not k.startswith("encoder.")}
    res = m.load_state_dict(own, strict=False)
    assert not res.unexpected_keys and all(k.startswith("encoder.") for k in res.missing_keys)
    for k, v in m.state_dict().items():
        assert torch.equal(v, torch.from_numpy(sd[k])), k
    m = m.to(dtype)
    m.encoder.pos = m.encoder.pos.to(dtype)
    m.temperature = m.temperature.to(dtype)
    return m, spec, sd


def grads_of(m, res, pre):
    none = []
    for k, p in m.named_parameters():
        if p.grad is None:
            none.append(k)
        else:
            res[pre + "grad." + k] = p.grad.detach().double().numpy().copy()
    return none


def run(mod, TestLoss, name, dtype):
    cfg = CASES[name]
    mod.np = _Float64Numpy() if dtype == torch.float64 else np
    try:
        return _run(mod, TestLoss, name, cfg, dtype)
    finally:
        mod.np = np


def _run(mod, TestLoss, name, cfg, dtype):
    res, extra = {}, {}
    loss_fn = TestLoss(size_average=False)
    pos, fx, y, yy = (torch.from_numpy(a).to(dtype) for a in R.draw_inputs(cfg, GEOM, TRAIN["Tout"]))
    B = cfg["B"]
    m, spec, sd = build(mod, cfg, dtype)
    assert "temperature" not in dict(m.named_parameters()) and "temperature" not in m.state_dict()
    extra["spec"], extra["sd"] = spec, sd
    pre = name + "."

    def predicted(model, key):
        zero(model)
        out = model(pos, fx, y, use_gt=False)
        loss = loss_fn(out.reshape(B, -1), y.reshape(B, -1))
        loss.backward()
        res[key + "out"] = out.detach().double().numpy()
        res[key + "slice_weights"] = model.slice_weights.detach().double().numpy()
        res[key + "code"] = model.code.detach().double().numpy()
        res[key + "loss"] = np.asarray(float(loss.detach()))
        extra[key + "no_grad"] = grads_of(model, res, key)

    predicted(m, pre + "pred.")
    mean_max = float(torch.from_numpy(res[pre + "pred.slice_weights"]).max(-1).values.mean())
    extra[pre + "mean_largest_weight"] = mean_max
    assert 0.3 <= mean_max <= 0.9, f"mean largest slice weight {mean_max:.3f} outside [0.3, 0.9]: adjust SLICE_SCALE"
    with torch.no_grad():
        res[pre + "get_code"] = m.get_code(pos, fx, y).double().numpy()
    if name == "a":
        with torch.no_grad():
            gt = m(pos, fx, y, use_gt=True)
        assert torch.equal(gt, torch.from_numpy(res[pre + "pred.out"]).to(dtype)), "use_gt=True gives another output"
        res[pre + "gt.out"] = gt.double().numpy()
        m.eval()
        with torch.no_grad():      # the evaluation loop of the reference's train(eval=True)
            w, step_loss, preds = fx, 0.0, []
            for t in range(TRAIN["Tout"]):
                yt = yy[..., t:t + 1]
                im = m(pos, w, yt, use_gt=False)
                step_loss += float(loss_fn(im.reshape(B, -1), yt.reshape(B, -1)))
                preds.append(im)
                w = torch.cat((w[..., 1:], im), dim=-1)
            pred = torch.cat(preds, -1)
            res[pre + "rollout.pred"] = pred.double().numpy()
            res[pre + "rollout.step_loss"] = np.asarray(step_loss)
            res[pre + "rollout.full_loss"] = np.asarray(float(loss_fn(pred.reshape(B, -1), yy.reshape(B, -1))))
        mt, _, _ = build(mod, cfg, dtype)
        opt = torch.optim.AdamW(mt.parameters(), lr=TRAIN["lr"], weight_decay=TRAIN["weight_decay"])
        sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=TRAIN["lr"], epochs=TRAIN["epochs"],
                                                    steps_per_epoch=TRAIN["steps_per_epoch"])
        losses = []
        for _ in range(TRAIN["steps"]):
            mt.train()
            w, loss = fx, 0
            for t in range(TRAIN["Tout"]):
                yt = yy[..., t:t + 1]
                im = mt(pos, w, yt, use_gt=False)
                loss = loss + loss_fn(im.reshape(B, -1), yt.reshape(B, -1))
                w = torch.cat((w[..., 1:], yt), dim=-1)
            opt.zero_grad()
            loss.backward()
            opt.step()
            sched.step()
            losses.append(float(loss.detach()))
        res[pre + "train.losses"] = np.asarray(losses)
    m.train()
    m.freeze_attention()
    extra[pre + "frozen.names"] = [k for k, p in m.named_parameters() if not p.requires_grad and not k.startswith("encoder.")]
    predicted(m, pre + "frozen.")
    for k in (pre + "frozen.out", pre + "frozen.slice_weights", pre + "frozen.code"):      # equal to pred.*: not stored twice
        res.pop(k)
    return res, extra


def main():
    if not os.path.isdir(REF):
        sys.exit(f"{REF} not found: this generator runs only next to the reference checkout")
    TestLoss = import_reference()[3]
    real_ones = torch.ones
    torch.ones = lambda *a, device=None, **k: real_ones(*a, **k)      # the constructor's mask asks for device='cuda'
    import matplotlib.pyplot as plt
    plt.show = lambda *a, **k: None
    import SequenSolverMerged as mod
    out = {}
    sig = inspect.signature(mod.SequenSolver.__init__).parameters
    out["signature"] = np.array(json.dumps([[k, None if p.default is inspect.Parameter.empty else p.default]
                                            for k, p in sig.items() if k != "self"]))
    out["geometry"] = np.array(json.dumps(GEOM))
    out["slice_scale"] = np.array(json.dumps(SLICE_SCALE))
    out["train.hyper"] = np.array(json.dumps(TRAIN))
    for name, cfg in CASES.items():
        print(f"case {name}: {cfg}")
        r64, extra = run(mod, TestLoss, name, torch.float64)
        r32, _ = run(mod, TestLoss, name, torch.float32)
        pre = name + "."
        spec, sd = extra["spec"], extra["sd"]
        out[pre + "config"] = np.array(json.dumps(cfg))
        out[pre + "keys"] = np.array([k for k, _ in spec])
        out[pre + "shapes"] = np.array(json.dumps([list(s) for _, s in spec]))
        out[pre + "sums"] = np.array([np.sum(sd[k], dtype=np.float64) for k, _ in spec])
        out[pre + "input_sums"] = np.array([np.sum(a, dtype=np.float64) for a in R.draw_inputs(cfg, GEOM, TRAIN["Tout"])])
        print(f"  mean largest slice weight {extra[pre + 'mean_largest_weight']:.3f}")
        for k, v in extra.items():
            if k.startswith(pre):
                out[k] = np.array(json.dumps(v))
        for k, v in r64.items():
            err = rel(r32[k], v)
            out["fp32_self_error." + k] = np.asarray(err)
            if k.endswith("slice_weights"):
                out[k + ".sum"] = np.asarray(np.sum(v, dtype=np.float64))
            if v.ndim == 0 or k.endswith("losses"):
                out[k] = v
            else:
                put(out, k, torch.from_numpy(np.ascontiguousarray(v)))
            bound = bound_of(k)
            flag = f"  -> bounded by 4 x self error = {4 * err:.2e}" if err > bound / 4 else ""
            print(f"  {k}: fp32 self error {err:.2e} (bound {bound:.0e}){flag}")
    path = os.path.join(GOLD, "G13_sequensolver_merged.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size <= 1_000_000, "the fixture must stay at or under 1 MB"


if __name__ == "__main__":
    main()
