"""Restatement of training-mode dropout for the tests — a helper module, not a test file.

* Philox4x32-10 and the draw contract in numpy: `philox4x32_10`, `draw_words`, `keep_mask`, `thresh_scale`.
* fp64 torch forwards with EXPLICIT masks, composed from the primitives of oracle/transolver_oracle.py (imported, not
  edited): `token_attention`, `attention_branch`, `model_forward` for the 2-D, 3-D and irregular models, and
  `layer_masks`, which lays the draws out in the order the package reserves them (blocks in model order; in each block
  the attention matrix [B, heads, M, M], then the to_out output [B, N, C]).
* `token_case`: the seeded inputs of the token-attention tests.

The reference applies dropout at two sites of a Physics-Attention layer (Physics_Attention.py:51,110,282 on the token
attention matrix after the softmax; the Dropout inside to_out, :28,85,257, before the block's residual add) and nowhere
else."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import transolver_oracle as orc

M0, M1 = 0xD2511F53, 0xCD9E8D57          # multipliers on counter words 0 and 2
W0, W1 = 0x9E3779B9, 0xBB67AE85          # key increments
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (anything numpy turns into uint64 arrays of 32-bit words) -> uint32 [..., 4]."""
    c = np.array(counter, dtype=np.uint64) & np.uint64(MASK32)
    k = np.array(key, dtype=np.uint64) & np.uint64(MASK32)
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = k[..., 0].copy(), k[..., 1].copy()
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # 32 x 32 -> 64 bits: no overflow in uint64
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        c0, c1, c2, c3 = n0, p1 & np.uint64(MASK32), n2, p0 & np.uint64(MASK32)
        k0, k1 = (k0 + np.uint64(W0)) & np.uint64(MASK32), (k1 + np.uint64(W1)) & np.uint64(MASK32)
    return np.stack((c0, c1, c2, c3), -1).astype(np.uint32)


def draw_words(seed, offset, n, first=0):
    """uint32 [n]: the words of the elements first .. first + n - 1 of the draw (seed, offset).  Element e takes word e & 3
    of philox(counter = (lo32(offset + e/4), hi32(offset + e/4), 0, 0), key = (lo32(seed), hi32(seed)))."""
    if n == 0:
        return np.zeros(0, dtype=np.uint32)
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    g0, g1 = first // 4, (first + n + 3) // 4
    c = np.full(g1 - g0, offset, dtype=np.uint64) + np.arange(g0, g1, dtype=np.uint64)      # wraps at 2^64 like the kernels
    counter = np.stack((c & np.uint64(MASK32), c >> np.uint64(32), np.zeros_like(c), np.zeros_like(c)), -1)
    key = np.broadcast_to(np.array([seed & MASK32, seed >> 32], dtype=np.uint64), (c.size, 2))
    words = philox4x32_10(counter, key).reshape(-1)
    return words[first - 4 * g0:first - 4 * g0 + n]


def keep_mask(seed, offset, n, thresh, first=0):
    """uint8 [n]: 1 where the element is kept (its word >= thresh)."""
    return (draw_words(seed, offset, n, first) >= np.uint32(thresh)).astype(np.uint8)


def thresh_scale(p):
    """(floor(p 2^32), fp32(1 / (1 - p)) as a Python float): what the kernels take."""
    return int(p * 2.0 ** 32), float(np.float32(1.0 / (1.0 - p)))


def layer_masks(seed, offset, thresh, n_layers, B, heads, M, N, C):
    """[(attention mask [B, heads, M, M], output mask [B, N, C])] per layer as float64 tensors, and the offset after them."""
    out = []
    for _ in range(n_layers):
        na, no = B * heads * M * M, B * N * C
        ma = keep_mask(seed, offset, na, thresh).reshape(B, heads, M, M)
        offset += (na + 3) // 4
        mo = keep_mask(seed, offset, no, thresh).reshape(B, N, C)
        offset += (no + 3) // 4
        out.append((torch.from_numpy(ma).double(), torch.from_numpy(mo).double()))
    return out, offset


# ----------------------------------------------------------------------------------------------- fp64 forwards
def token_attention(tok, wq, wk, wv, mask, scale):
    """orc.token_attention with the attention matrix dropped: softmax, then (.) mask * scale, then @ v."""
    D = tok.shape[-1]
    q, k, v = tok @ wq.t(), tok @ wk.t(), tok @ wv.t()
    a = torch.softmax((q @ k.transpose(-1, -2)) * D ** -0.5, dim=-1)
    return (a * mask * scale) @ v


def _conv3d(x, w, b, H, W, Dd):
    B, N, C = x.shape
    img = x.reshape(B, H, W, Dd, C).permute(0, 4, 1, 2, 3)
    return F.conv3d(img, w, b, padding=1).permute(0, 2, 3, 4, 1).reshape(B, N, -1)


def attention_branch(fx, sd, p, kind, geom, heads, masks, scale):
    """fx + dropout(to_out(deslice(dropout(attention))))) of block prefix `p` ("blocks.i."); kind: "2d" (geom = (H, W)),
    "3d" (geom = (H, W, D)) or "irregular" (geom None: Linear projections, temperature not clamped)."""
    a = p + "Attn."
    xn = orc.layer_norm(fx, sd[p + "ln_1.weight"], sd[p + "ln_1.bias"])
    wx, bx, wf, bf = (sd[a + k] for k in ("in_project_x.weight", "in_project_x.bias", "in_project_fx.weight",
                                            "in_project_fx.bias"))
    ws, bs, temp = sd[a + "in_project_slice.weight"], sd[a + "in_project_slice.bias"], sd[a + "temperature"]
    if kind == "2d":
        xm, fm = orc.conv3x3(xn, wx, bx, *geom), orc.conv3x3(xn, wf, bf, *geom)
    elif kind == "3d":
        xm, fm = _conv3d(xn, wx, bx, *geom), _conv3d(xn, wf, bf, *geom)
    else:
        xm, fm = xn @ wx.t() + bx, xn @ wf.t() + bf
    if kind == "irregular":
        w = torch.softmax((orc.split_heads(xm, heads) @ ws.t() + bs) / temp.reshape(1, -1, 1, 1), dim=-1)
        tok = (w.transpose(-1, -2) @ orc.split_heads(fm, heads)) / (w.sum(2) + orc.SLICE_EPS)[..., None]
    else:
        w, _, _, tok = orc.slice_tokens(xm, fm, ws, bs, temp, heads)
    o = token_attention(tok, sd[a + "to_q.weight"], sd[a + "to_k.weight"], sd[a + "to_v.weight"], masks[0], scale)
    z = orc.deslice(w, o) @ sd[a + "to_out.0.weight"].t() + sd[a + "to_out.0.bias"]
    return z * masks[1] * scale + fx


def embed(sd, x, fx, kind, cfg):
    """The input embedding (no dropout in it): what orc.model_forward / model_forward_irregular do before the blocks."""
    act = cfg.get("act", "gelu")
    if kind == "irregular":
        if cfg.get("unified_pos"):
            ref = cfg["ref"]
            r = torch.tensor(np.linspace(0, 1, ref), dtype=torch.float32).to(x.dtype)
            grid = torch.stack((r.reshape(ref, 1).expand(ref, ref), r.reshape(1, ref).expand(ref, ref)), -1).reshape(1, ref * ref, 2)
            x = torch.sqrt(((x[:, :, None, :] - grid[:, None, :, :]) ** 2).sum(-1))
        return orc.mlp(torch.cat((x, fx), -1) if fx is not None else x, sd, "preprocess.", act) + sd["placeholder"][None, None, :]
    assert not cfg.get("unified_pos"), "the structured restatements take the coordinates as they are"
    if fx is None:
        return orc.mlp(x, sd, "preprocess.", act) + sd["placeholder"][None, None, :]
    return orc.mlp(torch.cat((x, fx), -1), sd, "preprocess.", act)


def model_forward(sd, x, fx, kind, geom, cfg, masks, scale):
    """The model in training mode with dropout: `masks` from layer_masks; cfg needs n_head (and act, unified_pos, ref)."""
    heads, act = cfg["n_head"], cfg.get("act", "gelu")
    z = embed(sd, x, fx, kind, cfg)
    L = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    assert len(masks) == L
    for i in range(L):
        p = f"blocks.{i}."
        z = attention_branch(z, sd, p, kind, geom, heads, masks[i], scale)
        z = orc.mlp(orc.layer_norm(z, sd[p + "ln_2.weight"], sd[p + "ln_2.bias"]), sd, p + "mlp.", act) + z
    p = f"blocks.{L - 1}."
    return orc.layer_norm(z, sd[p + "ln_3.weight"], sd[p + "ln_3.bias"]) @ sd[p + "mlp2.weight"].t() + sd[p + "mlp2.bias"]


# ----------------------------------------------------------------------------------------------- test inputs
TOKEN_CASES = [(3, 8, 8, 2), (2, 12, 8, 3), (2, 64, 32, 2), (1, 128, 16, 2)]       # (BH, M, D, nchunk); the last is the LDS maximum
TOKEN_PS = (0.1, 0.5)
TOKEN_OFFSET = 2 ** 32 - 5            # the draws of the token tests cross the carry into the high counter word


def token_seed(BH, M, D, nchunk, p):
    return 7000 + 100 * M + D + int(10 * p)


def token_mask(BH, M, D, nchunk, p):
    """(mask uint8 [BH, M, M], rows [BH, M] that keep at least one element) of the case's draw."""
    thresh, _ = thresh_scale(p)
    mask = keep_mask(token_seed(BH, M, D, nchunk, p), TOKEN_OFFSET, BH * M * M, thresh).reshape(BH, M, M)
    return mask, mask.any(-1)


def token_case(BH, M, D, nchunk, seed):
    """fp32 numpy inputs of one token-attention case: the scatter's partial sums spart [BH, nchunk, M, D] and (positive)
    npart [BH, nchunk, M], the three [D, D] weights at the scale that keeps the softmax far from uniform, and the
    partials of dO [BH, nchunk, M, D]."""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    spart = f(BH, nchunk, M, D)
    npart = rng.uniform(0.5, 2.0, (BH, nchunk, M)).astype(np.float32)
    wq, wk, wv = (f(D, D) * np.float32(1.5 * D ** -0.5) for _ in range(3))
    return dict(spart=spart, npart=npart, wq=wq, wk=wk, wv=wv, dopart=f(BH, nchunk, M, D))


def token_reference(case, mask, scale):
    """fp64 (torch) outputs of token attention forward and backward for `token_case` inputs and an explicit mask
    [BH, M, M]: o, ds, dn, dwq, dwk, dwv.  s = sum of the partials, tokens = s / (n + eps); the gradients are autograd's."""
    t = {k: torch.from_numpy(v).double() for k, v in case.items()}
    s = t["spart"].sum(1).requires_grad_(True)
    n = t["npart"].sum(1).requires_grad_(True)
    w = [t[k].clone().requires_grad_(True) for k in ("wq", "wk", "wv")]
    o = token_attention(s / (n + orc.SLICE_EPS)[..., None], *w, torch.as_tensor(mask).double(), scale)
    ds, dn, dwq, dwk, dwv = torch.autograd.grad(o, [s, n] + w, t["dopart"].sum(1))
    return dict(o=o.detach(), ds=ds, dn=dn, dwq=dwq, dwk=dwk, dwv=dwv)
