"""Golden vectors of the previous-slice predictor: tests/golden/G23_previous_slice.npz.

Runs only where the reference checkout exists, on the CPU (like tools/make_golden_learnslice.py, whose conventions it
follows; `oracle.make_golden.import_reference()` installs the import shims).  It imports the reference's top-level
LearnSlice.py (class LearnSlice; the trainers behind `__main__` do not run) and calls ITS `forward_previous_slice` at its
hard-coded shape (prev_slice_weight [1, 1, 4096, 16], token [1, 1, 16, 32], weight_projection_form_slice = 528 -> 2112 ->
2112 -> 16) in float64 and in float32.

The weights (22 MB) are not stored: tests/previous_slice_restatement.draw_g23() fills them tensor by tensor from seeded
numpy.default_rng streams, here and in the tests, and the fixture records their sums.  Recorded:

  keys, shapes, sums            the six tensors of weight_projection_form_slice in state_dict order, and their float64 sums
  input_sums                    sums of (prev_slice_weight, token, target)
  point_stride, out.f64 / .f32  the output at every 7th point ([586, 16]) in both precisions; out.norm (float64, whole tensor)
  loss.f64 / .f32               one train_from_previous-style term, F.mse_loss(forward_previous_slice(prev, token), target)
                                (LearnSlice.py:744-745)
  whole_keys, grad.<key>        its float64 gradient of the three biases and of linear_post.weight, stored whole
  row_keys, row_stride,         every 97th row of the gradient of the two large matrices (linear_pre.0.weight [2112, 528],
  grad.<key>, grad.<key>.norm   linears.0.0.weight [2112, 2112]) with the norm of the whole gradient
  fp32_self_error.*             rel-L2 (loss: relative error) of the float32 run against the float64 run, per recorded item

Usage:  python tools/make_golden_previous_slice.py
"""
from __future__ import annotations

import json
import os
import sys

os.environ["MPLBACKEND"] = "Agg"

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))      # previous_slice_restatement.draw_g23: one definition for both sides

from oracle.make_golden import GOLD, REF, import_reference, rel  # noqa: E402
import previous_slice_restatement as R  # noqa: E402

STRIDE, ROW_STRIDE = 7, 97
P = R.PREFIX
WHOLE = (P + "linear_pre.0.bias", P + "linears.0.0.bias", P + "linear_post.bias", P + "linear_post.weight")
ROWS = (P + "linear_pre.0.weight", P + "linears.0.0.weight")


def run(ls_mod, sd, prev, token, target, dtype):
    """(output, loss, gradients by key) of the reference's module in `dtype`."""
    torch.set_default_dtype(dtype)
    try:
        m = ls_mod.LearnSlice(unified_pos=1, use_vorticity=1)
    finally:
        torch.set_default_dtype(torch.float32)
    m = m.to(dtype)
    res = m.load_state_dict({k: torch.from_numpy(v).to(dtype) for k, v in sd.items()}, strict=False)
    assert not res.unexpected_keys and not any(k.startswith(P) for k in res.missing_keys)
    m.train()
    out = m.forward_previous_slice(torch.from_numpy(prev).to(dtype), torch.from_numpy(token).to(dtype))
    assert out.dtype == dtype and tuple(out.shape) == (1, 1, 4096, 16)
    loss = F.mse_loss(out, torch.from_numpy(target).to(dtype))
    loss.backward()
    grads = {k: p.grad.detach() for k, p in m.named_parameters() if k.startswith(P)}
    return out.detach(), loss.detach(), grads


def main():
    if not os.path.isdir(REF):
        sys.exit(f"{REF} not found: this generator runs only next to the reference checkout")
    import_reference()
    import matplotlib.pyplot as plt
    plt.show = lambda *a, **k: None
    import LearnSlice as ls_mod
    sd, prev, token, target = R.draw_g23()
    shapes = R.previous_slice_shapes(R.G23_SHAPE["C"], R.G23_SHAPE["M"])
    out = {"keys": np.array([k for k, _ in shapes]), "shapes": np.array(json.dumps([list(s) for _, s in shapes])),
           "sums": np.array([np.sum(sd[k], dtype=np.float64) for k, _ in shapes]),
           "input_sums": np.array([np.sum(a, dtype=np.float64) for a in (prev, token, target)]),
           "point_stride": np.asarray(STRIDE), "row_stride": np.asarray(ROW_STRIDE),
           "whole_keys": np.array(WHOLE), "row_keys": np.array(ROWS)}
    o64, l64, g64 = run(ls_mod, sd, prev, token, target, torch.float64)
    o32, l32, g32 = run(ls_mod, sd, prev, token, target, torch.float32)
    out["out.f64"] = o64.numpy()[0, 0, ::STRIDE].astype(np.float64)
    out["out.f32"] = o32.numpy()[0, 0, ::STRIDE].astype(np.float32)
    out["out.norm"] = np.asarray(float(o64.norm()))
    out["fp32_self_error.out"] = np.asarray(rel(o32, o64))
    out["loss.f64"], out["loss.f32"] = np.asarray(float(l64)), np.asarray(float(l32))
    out["fp32_self_error.loss"] = np.asarray(abs(float(l32) - float(l64)) / abs(float(l64)))
    for k in WHOLE:
        out["grad." + k] = g64[k].numpy().astype(np.float64)
        out["fp32_self_error.grad." + k] = np.asarray(rel(g32[k], g64[k]))
    for k in ROWS:
        out["grad." + k] = g64[k].numpy()[::ROW_STRIDE].astype(np.float64)
        out["grad." + k + ".norm"] = np.asarray(float(g64[k].norm()))
        out["fp32_self_error.grad." + k] = np.asarray(rel(g32[k], g64[k]))
    for k in sorted(out):
        if k.startswith("fp32_self_error."):
            print(f"  {k}: {float(out[k]):.3g}")
    print(f"  loss {float(l64):.9g}, output norm {float(o64.norm()):.6g}")
    path = os.path.join(GOLD, "G23_previous_slice.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size <= 1_000_000, "the fixture must stay at or under 1 MB"


if __name__ == "__main__":
    main()
