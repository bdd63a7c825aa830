"""Golden vectors of the structured 2-D auto-encoder family: tests/golden/G9_encoder.npz.

Runs only where the reference checkout exists (like tools/make_golden_3d.py, whose conventions it follows and whose
helpers it reuses; `oracle.make_golden.import_reference()` installs the import shims, among them Tensor.cuda -> identity,
which covers the `.cuda()` of the reference's get_grid).  It imports the reference's
model/Transolver_Structured_Mesh2D_Encoder.Model and model/Physics_Attention.Physics_Attention_Structured_Mesh_2D_Auto_Encoder,
runs them in float64 on float32-representable weights and inputs (weights from synth.synth_state_dict_from_spec(keys/shapes,
seed); the fixture keeps keys, shapes, seeds and sums) and records (loss: the reference's TestLoss(size_average=False)):

  tiny_<variant>  the full model, B=2, H x W = 6 x 5, C=32, 4 heads, M=8, 2 layers, mlp_ratio=2, out_dim=2, temperatures
                  outside [0.1, 5]: `up` unified_pos=1, ref=4; `nofx` the fx=None placeholder branch; `time` the Time_Input
                  branch.  Inputs, output, loss, every parameter gradient, and the names of the parameters without one.
  seq.*           the stateful sequence on the `nofx`-shaped model with fx given (seed 34): encode -> code, slice;
                  decode -> y1, slice1; decode -> y2 (P(P(sw))); set_attention_slice(S) with a seeded non-softmax S ->
                  decode -> y3.  Then, from a fresh encode, the gradients of TestLoss(y1, target) with respect to every
                  parameter and to the code; and with every parameter frozen, the gradient with respect to the code alone.
  attn_<case>     the attention module alone, B=2 on 16 x 12: `m32` C=64, 8 heads (D=8), M=32; `m128` C=64, 4 heads
                  (D=16), M=128.  code = encode(x, cache_slice=True), the cached slice weights, out = reconstruct_fx(code)
                  + decode(code) (the last block's attention term), and the gradients of sum(out * gy) with respect to x
                  and every parameter.  x and gy: np.random.default_rng(seed + 100), checked by their sums.
  adamw.*         three iterations of auto_encoder.py's loop (model(x, fx) against fx, optimizer.zero_grad, backward,
                  clip_grad_norm_(1.0), AdamW(lr=1e-3, weight_decay=1e-5).step; constant lr) on a 2-layer model: the
                  three losses.
  signature       the reference Model's constructor parameters and defaults (JSON).

Usage:  python tools/make_golden_encoder.py
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle.make_golden import GOLD, REF, import_reference  # noqa: E402
from make_golden_3d import put, put_weights  # noqa: E402

TINY = dict(space_dim=2, n_layers=2, n_hidden=32, dropout=0.0, n_head=4, act='gelu', mlp_ratio=2, fun_dim=1, out_dim=2,
            slice_num=8, ref=4, H=6, W=5)
VARIANTS = {           # name: (constructor overrides, fx given, T given, weight seed)
    "up": (dict(unified_pos=1, Time_Input=False), True, False, 31),
    "nofx": (dict(unified_pos=0, Time_Input=False), False, False, 32),
    "time": (dict(unified_pos=0, Time_Input=True), True, True, 33),
}
SEQ_SEED = 34
ATTN = {               # name: (H, W, C, heads, M, B, seed)
    "m32": (16, 12, 64, 8, 32, 2, 41),
    "m128": (16, 12, 64, 4, 128, 2, 42),
}
ADAMW = dict(seed=35, steps=3, lr=1e-3, weight_decay=1e-5, clip=1.0)


def emb64(t, dim, max_period=10000):
    half = dim // 2
    freqs = torch.exp(-math.log(max_period) * torch.arange(half, dtype=torch.float64) / half)
    args = t[:, None].double() * freqs[None]
    return torch.cat([torch.cos(args), torch.sin(args)], dim=-1)


def make_model(Model, cfg, out, pre, seed):
    torch.manual_seed(seed)
    m = Model(**cfg)
    put_weights(out, pre, m, seed, wild=True)
    m = m.double()
    if cfg.get("unified_pos"):
        m.pos = m.pos.double()
    return m


def inputs(cfg, seed, with_fx, B=2):
    N = cfg["H"] * cfg["W"]
    rng = np.random.default_rng(seed + 100)
    nx = cfg["space_dim"] + (0 if with_fx else cfg["fun_dim"])
    x = rng.standard_normal((B, N, nx)).astype(np.float32)
    fx = rng.standard_normal((B, N, cfg["fun_dim"])).astype(np.float32) if with_fx else None
    y = rng.standard_normal((B, N, cfg["out_dim"])).astype(np.float32)
    return x, fx, y


def d(a):
    return None if a is None else torch.from_numpy(a).double()


def tiny(Model, mod, TestLoss, out):
    for name, (over, with_fx, with_T, seed) in VARIANTS.items():
        cfg = dict(TINY, **over)
        pre = f"tiny_{name}."
        m = make_model(Model, cfg, out, pre, seed)
        x, fx, y = inputs(cfg, seed, with_fx)
        B = x.shape[0]
        T = np.array([[0.25], [3.0]], dtype=np.float32) if with_T else None
        emb = mod.timestep_embedding
        if with_T:      # the same formula in float64 (the reference's casts to float32)
            mod.timestep_embedding = emb64
        try:
            pred = m(d(x), d(fx), T=d(T))
        finally:
            mod.timestep_embedding = emb
        loss = TestLoss(size_average=False)(pred.reshape(B, -1), d(y).reshape(B, -1))
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
        none = []
        for k, p in m.named_parameters():
            if p.grad is None:
                none.append(k)
            else:
                put(out, pre + "grad." + k, p.grad)
        out[pre + "no_grad"] = np.array(json.dumps(none))
        print(f"  {pre} loss {float(loss.detach()):.6f}, |pred| {float(pred.norm()):.4f}, no grad: {none}")


def sequence(Model, TestLoss, out):
    cfg = dict(TINY, unified_pos=0, Time_Input=False)
    pre = "seq."
    m = make_model(Model, cfg, out, pre, SEQ_SEED)
    x, fx, y = inputs(cfg, SEQ_SEED, True)
    B, N = x.shape[0], x.shape[1]
    heads, M = cfg["n_head"], cfg["slice_num"]
    out[pre + "config"] = np.array(json.dumps(cfg))
    out[pre + "x"], out[pre + "fx"], out[pre + "y"] = x, fx, y
    with torch.no_grad():
        code = m.encode(d(x), d(fx))
        put(out, pre + "code", code)
        put(out, pre + "slice0", m.get_attention_slice())
        put(out, pre + "y1", m.decode(code))
        put(out, pre + "slice1", m.get_attention_slice())
        put(out, pre + "y2", m.decode(code))
        put(out, pre + "slice2", m.get_attention_slice())
        S = (np.random.default_rng(SEQ_SEED + 200).standard_normal((B, heads, N, M)) * 0.3).astype(np.float32)
        out[pre + "S"] = S
        m.set_attention_slice(d(S))
        put(out, pre + "y3", m.decode(code))
    # gradients of a loss on y1 (fresh encode): every parameter and the code
    code = m.encode(d(x), d(fx))
    code.retain_grad()
    y1 = m.decode(code)
    loss = TestLoss(size_average=False)(y1.reshape(B, -1), d(y).reshape(B, -1))
    loss.backward()
    out[pre + "loss1"] = np.asarray(float(loss.detach()))
    put(out, pre + "dcode", code.grad)
    none = []
    for k, p in m.named_parameters():
        if p.grad is None:
            none.append(k)
        else:
            put(out, pre + "grad." + k, p.grad)
    out[pre + "no_grad"] = np.array(json.dumps(none))
    # frozen encoder (SequenSolver): parameters without gradients, the code is the only leaf
    for p in m.parameters():
        p.requires_grad_(False)
        p.grad = None
    with torch.no_grad():
        code = m.encode(d(x), d(fx))
    code = code.clone().requires_grad_(True)
    y1 = m.decode(code)
    TestLoss(size_average=False)(y1.reshape(B, -1), d(y).reshape(B, -1)).backward()
    put(out, pre + "dcode_frozen", code.grad)
    print(f"  {pre} loss1 {float(loss.detach()):.6f}, |dcode| {float(out[pre + 'dcode'].__array__().std()):.4g}, "
          f"no grad: {none}")


def attn(Attn, out):
    for name, (H, W, C, heads, M, B, seed) in ATTN.items():
        pre = f"attn_{name}."
        torch.manual_seed(seed)
        a = Attn(C, heads=heads, dim_head=C // heads, dropout=0.0, slice_num=M, H=H, W=W)
        put_weights(out, pre, a, seed, wild=True)
        a = a.double()
        N = H * W
        rng = np.random.default_rng(seed + 100)
        x = rng.standard_normal((B, N, C)).astype(np.float32)
        gy = rng.standard_normal((B, N, C)).astype(np.float32)
        xt = torch.from_numpy(x).double().requires_grad_(True)
        code = a.encode(xt, cache_slice=True)
        sw = a.slice_weights
        yv = a.reconstruct_fx(code) + a.decode(code)
        yv.backward(torch.from_numpy(gy).double())
        out[pre + "geom"] = np.array([H, W, C, heads, M, B])
        out[pre + "x.sum"] = np.asarray(np.sum(x, dtype=np.float64))
        out[pre + "gy.sum"] = np.asarray(np.sum(gy, dtype=np.float64))
        put(out, pre + "code", code)
        put(out, pre + "sw", sw)
        put(out, pre + "y", yv)
        put(out, pre + "dx", xt.grad)
        for k, p in a.named_parameters():
            put(out, pre + "grad." + k, p.grad)
        print(f"  {pre} |y| {float(yv.norm()):.4f}, |dx| {float(xt.grad.norm()):.4f}")


def adamw(Model, TestLoss, out):
    cfg = dict(TINY, unified_pos=0, Time_Input=False, fun_dim=2, out_dim=2)
    pre = "adamw."
    seed = ADAMW["seed"]
    m = make_model(Model, cfg, out, pre, seed)
    x, fx, _ = inputs(cfg, seed, True)
    B = x.shape[0]
    opt = torch.optim.AdamW(m.parameters(), lr=ADAMW["lr"], weight_decay=ADAMW["weight_decay"])
    losses = []
    for _ in range(ADAMW["steps"]):
        im = m(d(x), fx=d(fx))
        loss = TestLoss(size_average=False)(im.reshape(B, -1), d(fx).reshape(B, -1))
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), ADAMW["clip"])
        opt.step()
        losses.append(float(loss.detach()))
    out[pre + "config"] = np.array(json.dumps(cfg))
    out[pre + "hyper"] = np.array(json.dumps(ADAMW))
    out[pre + "x"], out[pre + "fx"] = x, fx
    out[pre + "losses"] = np.array(losses)
    print(f"  {pre} losses {losses}")


def main():
    if not os.path.isdir(REF):
        sys.exit(f"{REF} not found: this generator runs only next to the reference checkout")
    TestLoss = import_reference()[3]      # shims (timm stub, Tensor.cuda -> identity), the reference on sys.path
    import model.Transolver_Structured_Mesh2D_Encoder as mod
    from model.Physics_Attention import Physics_Attention_Structured_Mesh_2D_Auto_Encoder as Attn
    Model = mod.Model
    out = {}
    sig = inspect.signature(Model.__init__).parameters
    out["signature"] = np.array(json.dumps([[k, p.default] for k, p in sig.items() if k != "self"]))
    torch.manual_seed(0)
    out["name"] = np.array(Model(**dict(TINY, unified_pos=1)).__name__)
    tiny(Model, mod, TestLoss, out)
    sequence(Model, TestLoss, out)
    attn(Attn, out)
    adamw(Model, TestLoss, out)
    path = os.path.join(GOLD, "G9_encoder.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
