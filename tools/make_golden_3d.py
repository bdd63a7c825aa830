"""Golden vectors of the structured 3-D mesh family: tests/golden/G8_structured3d.npz.

Runs only where the reference checkout exists (like oracle/make_golden.py, whose import shims it reuses:
`oracle.make_golden.import_reference()`).  It imports the reference's model/Transolver_Structured_Mesh_3D.Model and
model/Physics_Attention.Physics_Attention_Structured_Mesh_3D, runs them in float64 on float32-representable weights and
inputs, and records what they produce (loss: the reference's TestLoss(size_average=False)):

  tiny_<variant>  the full model, B=2, (H, W, D) = (4, 5, 3), C=32, 4 heads, M=8, 2 layers, mlp_ratio=2, out_dim=2, with
                  temperatures outside [0.1, 5] (clamp mask): `up` unified_pos=1, ref=4; `nofx` unified_pos=0 and the
                  fx=None placeholder branch; `time` the Time_Input branch.  Inputs, output, the summed rel-L2 loss and
                  every parameter gradient.
  attn_<shape>    Physics_Attention_Structured_Mesh_3D alone: (8, 8, 8), C=64, 8 heads, M=16, B=2; and the degenerate
                  extents (1, 6, 5), (3, 1, 7) at C=32, 4 heads, M=8, B=2.  Output, input gradient, parameter gradients.
  pos             the reference's own get_grid() at (4, 5, 3), ref=4 (float32).
  signature       the reference Model's constructor parameters and defaults (JSON).

Weights are not stored: they come from `synth.synth_state_dict_from_spec(keys/shapes, seed)` (numpy's seeded generator,
the same on every host); the fixture keeps the keys, shapes, seeds and the float64 sum of every tensor so that a test can
check that it regenerated the same values; so are the inputs of the attention cases (x, then the output gradient gy:
`np.random.default_rng(seed + 100).standard_normal((B, N, C))` in float32).  Tensors larger than SMALL elements are stored as a strided sample plus their
norm (as tests/golden/G2_attn_ns.npz does).  The reference computes its time embedding in float32; the `time` variant
replaces that one function of the reference module by the same formula in float64 (harness-side, nothing is edited).

Usage:  python tools/make_golden_3d.py
"""
from __future__ import annotations

import inspect
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.make_golden import GOLD, REF, import_reference  # noqa: E402
from transformerbasednavierstokesolver_amd import synth  # noqa: E402

SMALL = 2048          # tensors up to this many elements are stored whole
SAMPLE = 1031         # otherwise: about this many elements at a fixed stride, plus the norm
TINY = dict(space_dim=3, n_layers=2, n_hidden=32, dropout=0.0, n_head=4, act='gelu', mlp_ratio=2, fun_dim=1, out_dim=2,
            slice_num=8, ref=4, H=4, W=5, D=3)
VARIANTS = {           # name: (constructor overrides, fx given, T given, weight seed)
    "up": (dict(unified_pos=1, Time_Input=False), True, False, 31),
    "nofx": (dict(unified_pos=0, Time_Input=False), False, False, 32),
    "time": (dict(unified_pos=0, Time_Input=True), True, True, 33),
}
ATTN = {               # name: (H, W, D, C, heads, M, B, seed)
    "8x8x8": (8, 8, 8, 64, 8, 16, 2, 41),
    "1x6x5": (1, 6, 5, 32, 4, 8, 2, 42),
    "3x1x7": (3, 1, 7, 32, 4, 8, 2, 43),
}


def put(out, key, t):
    """Whole tensor if small, else `<key>.sample` / `<key>.stride` / `<key>.norm` (the norm in float64; values rounded
    to float32, 6e-8 relative: far below every tolerance the fixture is used with)."""
    a = np.asarray(t.detach().double().numpy() if torch.is_tensor(t) else t, dtype=np.float64)
    if a.size <= SMALL:
        out[key] = a.astype(np.float32)
        return
    stride = a.size // SAMPLE
    out[key + ".sample"] = a.ravel()[::stride][:SAMPLE].astype(np.float32)
    out[key + ".stride"] = np.asarray(stride)
    out[key + ".norm"] = np.asarray(np.linalg.norm(a))


def put_weights(out, pre, m, seed, wild):
    spec = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    sd = synth.synth_state_dict_from_spec(spec, seed=seed, wild_temperature=wild)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    out[pre + "keys"] = np.array([k for k, _ in spec])
    out[pre + "shapes"] = np.array(json.dumps([list(s) for _, s in spec]))
    out[pre + "sums"] = np.array([np.sum(sd[k], dtype=np.float64) for k, _ in spec])
    out[pre + "seed"] = np.asarray(seed)
    return sd


def tiny(Model, mod, TestLoss, out):
    for name, (over, with_fx, with_T, seed) in VARIANTS.items():
        cfg = dict(TINY, **over)
        pre = f"tiny_{name}."
        torch.manual_seed(seed)
        m = Model(**cfg)
        put_weights(out, pre, m, seed, wild=True)
        m = m.double()
        if cfg["unified_pos"]:
            m.pos = m.pos.double()
        B, N = 2, cfg["H"] * cfg["W"] * cfg["D"]
        rng = np.random.default_rng(seed + 100)
        nx = cfg["space_dim"] + (0 if with_fx else cfg["fun_dim"])
        x = rng.standard_normal((B, N, nx)).astype(np.float32)
        fx = rng.standard_normal((B, N, cfg["fun_dim"])).astype(np.float32) if with_fx else None
        y = rng.standard_normal((B, N, cfg["out_dim"])).astype(np.float32)
        T = np.array([[0.25], [3.0]], dtype=np.float32) if with_T else None
        emb = mod.timestep_embedding
        if with_T:      # the same formula in float64 (the reference's casts to float32)
            def emb64(t, dim, max_period=10000):
                half = dim // 2
                freqs = torch.exp(-math.log(max_period) * torch.arange(half, dtype=torch.float64) / half)
                args = t[:, None].double() * freqs[None]
                return torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
            mod.timestep_embedding = emb64
        try:
            pred = m(torch.from_numpy(x).double(), None if fx is None else torch.from_numpy(fx).double(),
                     T=None if T is None else torch.from_numpy(T).double())
        finally:
            mod.timestep_embedding = emb
        loss = TestLoss(size_average=False)(pred.reshape(B, -1), torch.from_numpy(y).double().reshape(B, -1))
        loss.backward()
        out[pre + "config"] = np.array(json.dumps(cfg))
        out[pre + "x"] = x
        if fx is not None:
            out[pre + "fx"] = fx
        if T is not None:
            out[pre + "T"] = T
        out[pre + "y"] = y
        put(out, pre + "pred", pred)
        out[pre + "loss"] = np.asarray(float(loss.detach()))
        for k, p in m.named_parameters():
            if p.grad is not None:        # the placeholder takes no part when fx is given: no gradient, no entry
                put(out, pre + "grad." + k, p.grad)
        print(f"  {pre} loss {float(loss.detach()):.6f}, |pred| {float(pred.norm()):.4f}")


def attn(Attn, out):
    for name, (H, W, D, C, heads, M, B, seed) in ATTN.items():
        pre = f"attn_{name}."
        torch.manual_seed(seed)
        a = Attn(C, heads=heads, dim_head=C // heads, dropout=0.0, slice_num=M, H=H, W=W, D=D)
        put_weights(out, pre, a, seed, wild=True)
        a = a.double()
        N = H * W * D
        rng = np.random.default_rng(seed + 100)
        x = rng.standard_normal((B, N, C)).astype(np.float32)
        gy = rng.standard_normal((B, N, C)).astype(np.float32)
        xt = torch.from_numpy(x).double().requires_grad_(True)
        yv = a(xt)
        yv.backward(torch.from_numpy(gy).double())
        out[pre + "geom"] = np.array([H, W, D, C, heads, M, B])
        out[pre + "x.sum"] = np.asarray(np.sum(x, dtype=np.float64))     # x, gy: regenerated from the seed
        out[pre + "gy.sum"] = np.asarray(np.sum(gy, dtype=np.float64))
        put(out, pre + "y", yv)
        put(out, pre + "dx", xt.grad)
        for k, p in a.named_parameters():
            put(out, pre + "grad." + k, p.grad)
        print(f"  {pre} |y| {float(yv.norm()):.4f}, |dx| {float(xt.grad.norm()):.4f}")


def main():
    if not os.path.isdir(REF):
        sys.exit(f"{REF} not found: this generator runs only next to the reference checkout")
    TestLoss = import_reference()[3]      # shims (timm stub, Tensor.cuda -> identity), the reference on sys.path
    import model.Transolver_Structured_Mesh_3D as mod
    from model.Physics_Attention import Physics_Attention_Structured_Mesh_3D as Attn
    Model = mod.Model
    out = {}
    sig = inspect.signature(Model.__init__).parameters
    out["signature"] = np.array(json.dumps([[k, p.default] for k, p in sig.items() if k != "self"]))
    torch.manual_seed(0)
    m = Model(**dict(TINY, unified_pos=1))
    pos = m.pos.detach().numpy()
    assert pos.dtype == np.float32 and pos.shape == (1, 4, 5, 3, 64)
    out["pos_4x5x3_ref4"] = pos
    out["name"] = np.array(m.__name__)
    tiny(Model, mod, TestLoss, out)
    attn(Attn, out)
    path = os.path.join(GOLD, "G8_structured3d.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
