"""Golden vectors of training-mode dropout: tests/golden/G24_dropout.npz.

Runs only where the reference checkout exists, on the CPU (like oracle/make_golden.py, whose import shims it reuses:
`oracle.make_golden.import_reference()`).  It builds the reference's 2-D structured model at the shape of G1 (synth.TINY_CONFIG:
B=2, 6 x 5 mesh, C=32, 4 heads, M=12, 2 layers; coordinates as given instead of the unified-position grid, whose float32 square
roots differ in the last bit between hosts; temperatures outside [0.1, 5]) and its irregular-mesh model at the shape of G6's
`tiny` case, both with dropout=0.25 and in training mode, and replaces ON THE INSTANCES each nn.Dropout member of a layer
(`Attn.dropout`, `Attn.to_out[1]`) by a module that multiplies by a given mask and by fp32(1 / (1 - p)); no reference text
is edited or copied.  The masks are the package's draws (tests/dropout_restatement.py: Philox4x32-10 from SEED, offset 0,
blocks in model order, in each block the attention matrix [B, heads, M, M] and then the to_out output [B, N, C]).

Recorded per case `<tag>.` (tags `2d`, `irregular`): config (JSON), seed, p, thresh, scale, the masks (uint8), the inputs x,
fx and the output gradient gy, the state_dict, the output in fp32 and fp64 and the fp64 gradient of sum(out * gy) for
every parameter that has one.

Usage:  python tools/make_golden_dropout.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.make_golden import GOLD, import_reference  # noqa: E402
from transformerbasednavierstokesolver_amd import synth  # noqa: E402
import dropout_restatement as dr  # noqa: E402

SEED, P = 20241, 0.25
CASES = {      # tag: (config, B, N, weight seed)
    "2d": (dict(synth.TINY_CONFIG, unified_pos=0, dropout=P), 2, 30, 241),
    "irregular": (synth.make_config(n_layers=2, n_hidden=32, n_head=4, slice_num=12, fun_dim=3, out_dim=2, unified_pos=1,
                                    ref=3, mlp_ratio=2, dropout=P), 2, 45, 113),
}


class MaskMul(torch.nn.Module):
    """Stands in for an nn.Dropout of the reference instance: x * mask * scale with a mask given from outside."""

    def __init__(self, mask, scale):
        super().__init__()
        self.mask, self.scale = mask, scale

    def forward(self, x):
        assert x.shape == self.mask.shape, (tuple(x.shape), tuple(self.mask.shape))
        return x * self.mask.to(x.dtype) * self.scale


def build(tag, cfg, sd, dtype, masks, scale, Model2D, ModelIrregular):
    kw = dict(space_dim=2, n_layers=cfg["n_layers"], n_hidden=cfg["n_hidden"], dropout=P, n_head=cfg["n_head"],
              Time_Input=False, mlp_ratio=cfg["mlp_ratio"], fun_dim=cfg["fun_dim"], out_dim=cfg["out_dim"],
              slice_num=cfg["slice_num"], ref=cfg["ref"], unified_pos=cfg["unified_pos"])
    m = Model2D(H=cfg["H"], W=cfg["W"], **kw) if tag == "2d" else ModelIrregular(**kw)
    res = m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    m = m.to(dtype).train()
    for blk, (ma, mo) in zip(m.blocks, masks):
        assert isinstance(blk.Attn.dropout, torch.nn.Dropout) and isinstance(blk.Attn.to_out[1], torch.nn.Dropout)
        blk.Attn.dropout = MaskMul(ma, scale)
        blk.Attn.to_out[1] = MaskMul(mo, scale)
    assert not any(isinstance(x, torch.nn.Dropout) for x in m.modules()), "a dropout site the masks do not cover"
    return m


def main():
    Model2D = import_reference()[0]
    from model.Transolver_Irregular_Mesh import Model as ModelIrregular
    thresh, scale = dr.thresh_scale(P)
    out = {}
    for tag, (cfg, B, N, wseed) in CASES.items():
        sd = (synth.synth_state_dict(cfg, seed=wseed, wild_temperature=True) if tag == "2d"
              else synth.synth_irregular_state_dict(cfg, seed=wseed))
        rng = np.random.default_rng(wseed + 1)
        x = rng.uniform(0, 1, (B, N, 2)).astype(np.float32)
        fx = rng.standard_normal((B, N, cfg["fun_dim"])).astype(np.float32)
        gy = rng.standard_normal((B, N, cfg["out_dim"])).astype(np.float32)
        masks, _ = dr.layer_masks(SEED, 0, thresh, cfg["n_layers"], B, cfg["n_head"], cfg["slice_num"], N, cfg["n_hidden"])
        pre = tag + "."
        out.update({pre + "config": np.asarray(json.dumps(cfg)), pre + "seed": np.asarray(SEED), pre + "p": np.asarray(P),
                    pre + "thresh": np.asarray(thresh, dtype=np.uint32), pre + "scale": np.asarray(scale, dtype=np.float32),
                    pre + "x": x, pre + "fx": fx, pre + "gy": gy})
        out.update({pre + "sd." + k: v for k, v in sd.items()})
        for i, (ma, mo) in enumerate(masks):
            out[f"{pre}mask.{i}.attn"], out[f"{pre}mask.{i}.out"] = ma.numpy().astype(np.uint8), mo.numpy().astype(np.uint8)
        for dtype, dt in ((torch.float64, "f64"), (torch.float32, "f32")):
            m = build(tag, cfg, sd, dtype, masks, scale, Model2D, ModelIrregular)
            pred = m(torch.from_numpy(x).to(dtype), torch.from_numpy(fx).to(dtype))
            out[f"{pre}pred.{dt}"] = pred.detach().numpy()
            if dt == "f64":
                pred.backward(torch.from_numpy(gy).to(dtype))
                for k, p in m.named_parameters():
                    if p.grad is not None:
                        out[f"{pre}grad.f64.{k}"] = p.grad.numpy()
        # the restatement reproduces the reference (tests/test_dropout_host.py re-checks it from the fixture)
        sdo = {k: torch.from_numpy(v).double() for k, v in sd.items()}
        ro = dr.model_forward(sdo, torch.from_numpy(x).double(), torch.from_numpy(fx).double(), tag,
                              (cfg["H"], cfg["W"]) if tag == "2d" else None, cfg, masks, scale)
        err = float((ro - torch.from_numpy(out[pre + "pred.f64"])).norm() / torch.from_numpy(out[pre + "pred.f64"]).norm())
        keep = np.mean([float(ma.mean()) for ma, _ in masks])
        print(f"{tag}: restatement vs reference rel-L2 {err:.2e}; attention keep fraction {keep:.3f}")
        assert err < 1e-12, tag
    path = os.path.join(GOLD, "G24_dropout.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
