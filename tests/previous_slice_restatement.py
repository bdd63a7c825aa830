"""Plain-torch restatement of the reference's previous-slice predictor (LearnSlice.forward_previous_slice, LearnSlice.py:
125-134) and of the EAGER loops of its three slice trainers (train :477-526, train_from_vorticity :929-962,
train_from_previous :722-755, and the evaluation loop :663-706), in whatever dtype its inputs have (helper module of the
suite, not a conftest).  The frozen sequence model is restated by sequensolver_restatement, the other two predictors by
learnslice_restatement / slicepredictor_restatement.  Test infrastructure only."""
from __future__ import annotations

import numpy as np
import torch

import learnslice_restatement as RL
import sequensolver_restatement as RP
import slicepredictor_restatement as RS

PREFIX = "weight_projection_form_slice."


def previous_slice_shapes(C=32, M=16):
    """[(key, shape)] of the reference's `weight_projection_form_slice = MLP(M + M C, 4 (M + M C), M, 1)`, in the order
    of its state_dict."""
    cat = M + M * C
    return RS._mlp_shapes(PREFIX, cat, 4 * cat, M, 1)


def forward_previous_slice(sd, prev_slice_weight, token):
    """The reference's lines, on the explicit concatenation: prev_slice_weight [B, 1, N, M], token [B, 1, M, C] -> the raw
    MLP output [B, 1, N, M] (any B: the flattened token of sample b goes to the N points of sample b)."""
    B, _, N, _ = prev_slice_weight.shape
    flat = token.reshape(B, 1, 1, -1).expand(-1, -1, N, -1)
    return RS.mlp(torch.cat((prev_slice_weight, flat), -1), sd, PREFIX, 1)


def forward_split(sd, prev_slice_weight, token):
    """The same layer with linear_pre's weight cut in two column blocks: the first M columns multiply the point's slice
    weights, the other M C the flattened token in (m, c) order, one row per sample."""
    import torch.nn.functional as F
    B, _, N, M = prev_slice_weight.shape
    w, b = sd[PREFIX + "linear_pre.0.weight"], sd[PREFIX + "linear_pre.0.bias"]
    tb = token.reshape(B, -1) @ w[:, M:].t() + b                                   # [B, H]
    h0 = F.gelu(prev_slice_weight.reshape(B, N, M) @ w[:, :M].t() + tb[:, None, :])
    h1 = F.gelu(h0 @ sd[PREFIX + "linears.0.0.weight"].t() + sd[PREFIX + "linears.0.0.bias"]) + h0
    return (h1 @ sd[PREFIX + "linear_post.weight"].t() + sd[PREFIX + "linear_post.bias"]).reshape(B, 1, N, M)


def mse(a, b):
    return ((a - b) ** 2).mean()


# ---------------------------------------------------------------------------------------------- the frozen sequence model
class Frozen:
    """get_code / encoder slice weights / decode of a SequenSolver state_dict (tensors of one dtype), without gradient."""

    def __init__(self, sd, enc_cfg, layers):
        enc, own = RP.split_state_dict(sd)
        self.enc = {k: v.detach() for k, v in enc.items()}
        self.own = {k: v.detach() for k, v in own.items()}
        self.cfg, self.layers = enc_cfg, layers

    @torch.no_grad()
    def slice_weights(self, x, frame):
        """The encoder's slice weights of one frame [B, N, 1] -> [B, 1, N, M]."""
        return RP.encode(self.enc, self.cfg, x, frame)[1]

    @torch.no_grad()
    def code(self, x, fx):
        """(get_code on the window fx [B, N, T], the slice weights of the window's last frame)."""
        B, _, T = fx.shape
        enc = [RP.encode(self.enc, self.cfg, x, fx[:, :, i:i + 1]) for i in range(T)]
        _, _, M, C = enc[0][0].shape
        tokens = torch.stack([c.reshape(B, M * C) for c, _ in enc], 1)
        return RP.tokens_to_code(self.own, tokens, self.layers, (M * C) ** -0.5).reshape(B, 1, M, C), enc[-1][1]

    @torch.no_grad()
    def predict(self, sw, code):
        """decode with `sw`, then mlp2(ln_3(.)) -> [B, N, 1]."""
        from oracle import transolver_oracle as orc
        o = self.own
        return orc.layer_norm(orc.deslice(sw, code), o["ln_3.weight"], o["ln_3.bias"]) @ o["mlp2.weight"].t() + o["mlp2.bias"]


# ---------------------------------------------------------------------------------------------- predictors by kind
def predict(kind, sd, x, fx, code, prev, geom):
    """The slice weights the `kind`'s model makes for one call.  kind: "learnslice" (use_vorticity = 1), "conv"
    (SliceLearner), "vorticity" (code-conditioned), "previous"."""
    if kind == "learnslice":
        return RL.get_slice_weight(sd, code, x, fx, use_vorticity=1)
    if kind == "conv":
        return RS.slice_learner(sd, x, fx, geom["H"], geom["W"])
    if kind == "vorticity":
        return RS.vorticity_learner(sd, x, fx, code, geom["H"], geom["W"])
    return forward_previous_slice(sd, prev, code)


def loss_term(kind, pred, target):
    """learnslice: the sum over the points of F.mse_loss (:499-510); the others: F.mse_loss over all elements."""
    return RL.slice_mse(pred, target) if kind == "learnslice" else mse(pred, target)


def train_step(kind, sd, frozen, x, fx, yy, geom, lr):
    """One batch of the kind's EAGER training loop with plain SGD(lr) on the tensors of `sd` that require a gradient:
    learnslice steps once per frame, the others sum the Tout terms and step once.  The window slides on with the true
    frame.  Returns the list of the detached per-frame losses (learnslice) or [the summed loss]."""
    params = [v for v in sd.values() if v.requires_grad]
    opt = torch.optim.SGD(params, lr=lr)
    losses, total = [], 0
    for t in range(yy.shape[-1]):
        y = yy[..., t:t + 1]
        target = frozen.slice_weights(x, y)
        code, prev = frozen.code(x, fx)
        term = loss_term(kind, predict(kind, sd, x, fx, code, prev, geom), target)
        if kind == "learnslice":
            opt.zero_grad()
            term.backward()
            opt.step()
            losses.append(term.detach())
        else:
            total = total + term
        fx = torch.cat((fx[..., 1:], y), -1)
    if kind != "learnslice":
        opt.zero_grad()
        total.backward()
        opt.step()
        losses.append(total.detach())
    return losses


@torch.no_grad()
def previous_rollout(sd, frozen, x, fx, nsteps):
    """:663-706: the raw prediction decodes the code and the result enters the window."""
    preds = []
    for _ in range(nsteps):
        code, prev = frozen.code(x, fx)
        pred = frozen.predict(forward_previous_slice(sd, prev, code), code)
        preds.append(pred)
        fx = torch.cat((fx[..., 1:], pred), -1)
    return torch.cat(preds, -1)


# ---------------------------------------------------------------------------------------------- G23 fixture access
G23_SHAPE = dict(B=1, N=4096, M=16, C=32)          # the reference's hard-coded shape
G23_SEED = 2300


def draw_g23():
    """(state_dict, prev_slice_weight [1, 1, 4096, 16], token [1, 1, 16, 32], target [1, 1, 4096, 16]) as float32 numpy
    arrays, tensor by tensor from seeded streams, exactly as tools/make_golden_previous_slice.py draws them: weights normal
    with std 1 / sqrt(fan_in), biases normal with std 0.1, the previous and target slice weights softmaxes over M of
    normal logits (x 2), the token normal."""
    s = G23_SHAPE
    sd = {}
    for i, (key, shape) in enumerate(previous_slice_shapes(s["C"], s["M"])):
        rng = np.random.default_rng(G23_SEED + i)
        scale = 0.1 if key.endswith("bias") else 1.0 / np.sqrt(shape[1])
        sd[key] = (rng.standard_normal(shape) * scale).astype(np.float32)
    rng = np.random.default_rng(G23_SEED + 100)

    def softmax(z):
        e = np.exp(z - z.max(-1, keepdims=True))
        return (e / e.sum(-1, keepdims=True)).astype(np.float32)

    prev = softmax(2.0 * rng.standard_normal((s["B"], 1, s["N"], s["M"])))
    token = rng.standard_normal((s["B"], 1, s["M"], s["C"])).astype(np.float32)
    target = softmax(2.0 * rng.standard_normal((s["B"], 1, s["N"], s["M"])))
    return sd, prev, token, target


def rel(a, b):
    a, b = torch.as_tensor(a).double().reshape(-1), torch.as_tensor(b).double().reshape(-1)
    return float((a.cpu() - b.cpu()).norm() / b.cpu().norm().clamp_min(1e-300))
