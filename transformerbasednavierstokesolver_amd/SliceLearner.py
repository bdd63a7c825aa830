"""Conv slice predictors — slice weights predicted from the flow itself: a `preprocess` MLP over the point features, one
3x3 conv, a projection to M logits, a clamped temperature and a softmax over M.

`SliceLearner` is the drop-in for the reference's top-level SliceLearner.py (class SliceLearner): `Linear(n_hidden, M)`
after the conv.  `VorticitySliceLearner` is the code-conditioned form that the reference keeps in two places, line for line
the same: `LearnSlice.forward_from_vorticity` (LearnSlice.py:155-193) and `SequenSolverMerged.SequenSolver.forward_slice`.
There the conv output and the flattened code are each z-scored over the whole tensor (batch included), concatenated and
sent through `in_project_slice = MLP(n_hidden + M*C, (n_hidden + M*C)//2, M)`.

Every stage is a libpa2d launch: the preprocess MLP (functional.mlp), the single conv (functional.conv3x3,
pa2d_conv3x3_*), the z-score (functional.zscore, pa2d_zscore_*), the dense layers (functional.linear) and the last layer
with its softmax (functional.wide_slice_weights, pa2d_wide_slice_weights_*).  The [B, N, n_hidden + M*C] tensor is never
formed: the first layer of the MLP separates into the row GEMM z(x_mid) . W1x^T and a per-sample row
tb[b] = z(code)[b] . W1c^T + b1, which is that GEMM's bias (one launch per sample; B is 1 in every reference use)."""
import numpy as np
import torch
import torch.nn as nn

from . import functional as Fn
from . import ops
from .model._core import ACTIVATION, MLP  # noqa: F401  (the reference module defines both names)


def _refuse_bf16_storage(engine):
    if engine is not None and ops.resolve_engine(engine) == ops.ENGINE_BF16S:
        raise NotImplementedError("bf16 storage (engine 'bf16s') is not implemented for the conv slice predictors")


class _EngineMixin:
    def set_engine(self, engine):
        """GEMM engine ("f32" | "split" | "bf16" | None = default) of the dense layers and the conv of THIS module; bf16
        storage ('bf16s') is refused.  The z-score and the wide slice weights are exact fp32 on every engine."""
        _refuse_bf16_storage(engine)
        eng = None if engine is None else ops.resolve_engine(engine)
        for m in self.modules():
            if hasattr(m, "engine"):
                m.engine = eng
        return self


class SliceLearner(_EngineMixin, nn.Module):
    """Reference SliceLearner.py, class SliceLearner: same constructor, names, order and defaults; forward(x, fx, T=None)
    returns the slice weights [B, 1, N, M].  `time_fc` exists with Time_Input (it is part of the state_dict) and, as in the
    reference, the forward never reads it or T."""

    def __init__(self, space_dim=1, n_hidden=256, Time_Input=False, act='gelu', fun_dim=1, ref=8, unified_pos=False, H=85,
                 W=85, slice_num=32):
        super().__init__()
        self.__name__ = 'Transolver_2D'
        self.H, self.W, self.ref, self.unified_pos = H, W, ref, unified_pos
        self.engine = None
        if unified_pos:
            # non-persistent buffer: follows .to() and stays out of the state_dict, like the reference's plain attribute
            self.register_buffer("pos", self.get_grid(), persistent=False)
        self.preprocess = MLP(fun_dim + (ref * ref if unified_pos else space_dim), n_hidden * 2, n_hidden, n_layers=0,
                              res=False, act=act)
        self.Time_Input, self.n_hidden, self.space_dim = Time_Input, n_hidden, space_dim
        if Time_Input:
            self.time_fc = nn.Sequential(nn.Linear(n_hidden, n_hidden), nn.SiLU(), nn.Linear(n_hidden, n_hidden))
        self.in_project_x = nn.Conv2d(n_hidden, n_hidden, 3, 1, 1)
        self.in_project_slice = nn.Linear(n_hidden, slice_num)
        self.temperature = nn.Parameter(torch.ones([1, 1, 1, 1]) * 0.5)
        self.initialize_weights()
        # created after the init pass, uniform in [0, 1/n_hidden) like the reference (:78)
        self.placeholder = nn.Parameter((1 / n_hidden) * torch.rand(n_hidden, dtype=torch.float))

    def initialize_weights(self):
        self.apply(self._init_weights)

    def _init_weights(self, m):
        """Linear: trunc_normal(std .02) / zero bias; LayerNorm: 1 / 0; Conv2d keeps PyTorch's default."""
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.zeros_(m.bias)
        elif isinstance(m, (nn.LayerNorm, nn.BatchNorm1d)):
            nn.init.ones_(m.weight)
            nn.init.zeros_(m.bias)

    def get_grid(self, batchsize=1):
        """[batchsize, H, W, ref*ref]: Euclidean distance of mesh point (i/(H-1), j/(W-1)) to the lattice point
        (k/(ref-1), l/(ref-1)), feature index k*ref+l; linspace in float64, arithmetic in float32."""
        axis = lambda n: torch.tensor(np.linspace(0, 1, n), dtype=torch.float)
        rows, cols, lat = axis(self.H), axis(self.W), axis(self.ref)
        dr2 = (rows[:, None] - lat[None, :]) ** 2           # H, ref
        dc2 = (cols[:, None] - lat[None, :]) ** 2           # W, ref
        pos = torch.sqrt(dr2[:, None, :, None] + dc2[None, :, None, :])
        return pos.reshape(1, self.H, self.W, self.ref ** 2).repeat(batchsize, 1, 1, 1).contiguous()

    def forward(self, x, fx, T=None):
        if self.unified_pos:      # the coordinates in `x` are ignored (only the batch size is used)
            x = self.pos.expand(x.shape[0], -1, -1, -1).reshape(x.shape[0], self.H * self.W, self.ref ** 2)
        if fx is not None:
            z = self.preprocess(torch.cat((x, fx), -1))
        else:
            z = self.preprocess(x) + self.placeholder[None, None, :]
        B, N, _ = z.shape
        if N != self.H * self.W:
            raise ValueError(f"this SliceLearner is built for a {self.H} x {self.W} mesh; got {N} points")
        x_mid = Fn.conv3x3(z, self.H, self.W, self.in_project_x.weight, self.in_project_x.bias, engine=self.engine)
        sw = Fn.wide_slice_weights(x_mid, self.temperature, self.in_project_slice.weight, self.in_project_slice.bias)
        return sw.reshape(B, 1, N, sw.shape[-1])


def code_conditioned_slice_weights(x, fx, code, preprocess, in_project_x, in_project_slice, temperature, H, W, M, C, engine,
                                   groups=1):
    """The reference's `LearnSlice.forward_from_vorticity` / merged `SequenSolver.forward_slice` over the caller's own
    sub-modules (the ONE implementation behind VorticitySliceLearner.forward and SequenSolverMerged.forward_slice):
    x [B, N, 64 or 2], fx [B, N, T], code [B, 1, M, C] or None -> slice weights [B, 1, N, M].  `preprocess` and
    `in_project_slice` are MLPs of model/_core.py, `in_project_x` a Conv2d(n_hidden, n_hidden, 3, 1, 1), `temperature` one
    scalar (a Parameter or a plain tensor).

    `groups` > 1: the batch holds `groups` independent calls of B / groups consecutive samples each (a time-folded
    iteration).  Both z-scores are then taken per group (functional.zscore(groups=...)), and the per-sample code term of the
    first layer is added to ONE row GEMM by the broadcast-add kernel (functional.embed_bias) before the activation.
    groups = 1 is the path as it was, per-sample loop included."""
    z = preprocess(torch.cat((x, fx), -1))
    B, N, nh = z.shape
    if N != H * W:
        raise ValueError(f"this predictor is built for a {H} x {W} mesh; got {N} points")
    x_mid = Fn.conv3x3(z, H, W, in_project_x.weight, in_project_x.bias, engine=engine)
    mlp = in_project_slice
    first, hidden, last = mlp.linear_pre[0], mlp.linears[0][0], mlp.linear_post
    act, eng = mlp.act_name, engine
    if code is None:
        h = Fn.linear(x_mid, first.weight, first.bias, act, engine=eng)
    else:
        if code.numel() != B * M * C:
            raise ValueError(f"need a code [B, 1, M, C] = {(B, 1, M, C)}; got {tuple(code.shape)}")
        if groups < 1 or B % groups:
            raise ValueError(f"groups = {groups} must divide the batch of {B}")
        zc = Fn.zscore(code.reshape(B, M * C), groups)
        zx = Fn.zscore(x_mid, groups)
        # first layer on cat(z(x_mid), z(code)) without the concatenation: the code term is one row per sample
        # (the two column blocks of the weight are cut out once per forward, not once per sample)
        w1x, w1c = first.weight[:, :nh].contiguous(), first.weight[:, nh:].contiguous()
        tb = Fn.linear(zc, w1c, first.bias, None, engine=eng)                             # [B, hidden]
        if groups > 1:  # a folded batch: ONE GEMM over all rows, the per-sample rows added by the broadcast-add kernel
            if tb.is_cuda and tb.shape[-1] % 4:      # Fn.embed_bias would take its torch expression: a missing kernel is an error
                raise NotImplementedError(f"the folded slice predictor needs a hidden width that is a multiple of 4 "
                                          f"(pa2d_embed_bias); got {tb.shape[-1]}")
            h = Fn.activation(Fn.embed_bias(Fn.linear(zx, w1x, None, None, engine=eng), None, tb), act)
        elif B == 1:    # every use in the reference: no per-sample pieces to put together
            h = Fn.linear(zx, w1x, tb[0], act, engine=eng)
        else:
            h = torch.stack([Fn.linear(zx[b], w1x, tb[b], act, engine=eng) for b in range(B)])
    y = Fn.linear(h, hidden.weight, hidden.bias, act, engine=eng)
    h = y + h if mlp.res else y
    sw = Fn.wide_slice_weights(h, temperature, last.weight, last.bias)
    return sw.reshape(B, 1, N, M)


class VorticitySliceLearner(_EngineMixin, nn.Module):
    """The code-conditioned conv predictor: forward(x, fx, code=None) is the reference's
    `LearnSlice.forward_from_vorticity` / merged `SequenSolver.forward_slice`.  x [B, N, 64 or 2] (the unified_pos distances
    or the coordinates), fx [B, N, T] (the last T frames), code [B, 1, M, C] -> slice weights [B, 1, N, M].

    The sub-modules carry the reference's names (`preprocess`, `in_project_x`, `in_project_slice`, `temperature`), so a
    reference LearnSlice or merged SequenSolver state_dict loads with strict=False and no missing key.  The first two
    constructor arguments are the reference's; C, M, T, H, W, n_hidden and act (keyword-only; the reference hard-codes
    32, 16, 10, 64, 64, 256 and 'gelu') are the extension.  Initialisation is PyTorch's default, as in the reference.

    `temperature` is a trainable Parameter here, as in SliceLearner.py.  In the reference's LearnSlice it stays 0.5: the
    `.cuda()` after `nn.Parameter(...)` returns a plain tensor, so the module never registers it and no optimizer sees it.

    fx=None raises ValueError: the reference reads a `placeholder` it never creates on that path."""

    def __init__(self, unified_pos=1, use_code_for_vorticity=True, *, C=32, M=16, T=10, H=64, W=64, n_hidden=256, act='gelu'):
        super().__init__()
        self.C, self.M, self.T, self.H, self.W, self.n_hidden = C, M, T, H, W, n_hidden
        self.unified_pos, self.use_code_for_vorticity = unified_pos, use_code_for_vorticity
        self.engine = None
        self.fundemental = T + (64 if unified_pos else 2)                                 # reference :74-78
        self.concatenated = n_hidden + (M * C if use_code_for_vorticity else 0)           # reference :79-82
        self.preprocess = MLP(self.fundemental, n_hidden * 2, n_hidden, n_layers=0, res=False, act=act)
        self.in_project_x = nn.Conv2d(n_hidden, n_hidden, 3, 1, 1)
        self.in_project_slice = MLP(self.concatenated, self.concatenated // 2, M)
        self.temperature = nn.Parameter(torch.ones([1, 1, 1, 1]) * 0.5)

    def forward(self, x, fx, code=None):
        return self.forward_folded(x, fx, code, 1)

    def forward_folded(self, x, fx, code=None, groups=1):
        """forward on a batch that holds `groups` independent calls of B / groups consecutive samples each (a time-folded
        iteration): the z-scores stay per call (code_conditioned_slice_weights).  groups = 1 is forward itself, the call as
        it was.  (A method of its own, not a keyword of forward, whose parameter list is the reference's.)"""
        if fx is None:
            raise ValueError("forward_from_vorticity needs fx: the reference's fx=None path reads a placeholder that its "
                             "LearnSlice never creates")
        if (code is not None) != bool(self.use_code_for_vorticity):
            raise ValueError(f"built with use_code_for_vorticity={self.use_code_for_vorticity}: in_project_slice takes "
                             f"{self.concatenated} features, so the code must be " +
                             ("given" if self.use_code_for_vorticity else "None"))
        args = (x, fx, code, self.preprocess, self.in_project_x, self.in_project_slice, self.temperature, self.H, self.W,
                self.M, self.C, self.engine)
        if groups == 1:         # the call as it was, argument list included: tests/test_sequensolver_merged_host.py replaces
            #                     the function by a stand-in of the former signature, which has no `groups`
            return code_conditioned_slice_weights(*args)
        return code_conditioned_slice_weights(*args, groups=groups)

    forward_from_vorticity = forward


# PreviousSliceLearner takes the fused first layer (functional.prev_slice_entry, pa2d_prev_slice_entry_*) by default only if
# its measured median lies outside the three-op route's range at n*B = 10 folded samples (the rule of DESIGN 4.17).
# Measured on the MI355X, forward plus backward, ms, median (min .. max) of 9: three-op 1.045 (1.038 .. 1.056), fused
# 0.451 (0.444 .. 0.458): outside, below.  `fused_entry = False` on a module selects the three-op route.
FUSED_ENTRY_DEFAULT = True


class PreviousSliceLearner(_EngineMixin, nn.Module):
    """The previous-slice predictor: forward(prev_slice_weight, token) is the reference's `LearnSlice.forward_previous_slice`
    (LearnSlice.py:125-134).  prev_slice_weight [B, 1, N, M] (the encoder's slice weights of the window's last frame, data),
    token [B, 1, M, C] (the code) -> the RAW output of `weight_projection_form_slice` [B, 1, N, M]: no softmax, as in the
    reference.  Any B (the reference's reshape is B = 1).

    The sub-module carries the reference's name, `weight_projection_form_slice = MLP(M + M C, 4 (M + M C), M, 1)`, so a
    reference LearnSlice state_dict loads with strict=False and no missing key.  Initialisation is PyTorch's default, as in
    the reference.  C, M and act (keyword-only; the reference hard-codes 32, 16 and 'gelu') are the extension.

    The [B, N, M + M C] concatenation is never formed.  The first M columns of linear_pre's weight multiply the point's
    slice weights; the other M C columns multiply the flattened token, in (m, c) order, which is the same for all N points:
        h0 = act(sw . Wsw^T + tb[b]),   tb = token.reshape(B, M C) . Wtok^T + bias    [B, H], H = 4 (M + M C)
        h1 = act(h0 . W1^T + b1) + h0,  out = h1 . Wpost^T + bpost
    tb and the two later layers are functional.linear on this module's engine; h0 is functional.prev_slice_entry:
    `fused_entry` True takes the fused kernels (exact fp32; one launch forward), False the row GEMM + broadcast add + activation."""

    def __init__(self, *, C=32, M=16, act='gelu'):
        super().__init__()
        self.C, self.M = C, M
        self.engine = None
        self.fused_entry = FUSED_ENTRY_DEFAULT
        self.concatenated = M + M * C                                                     # reference :66
        self.weight_projection_form_slice = MLP(self.concatenated, self.concatenated * 4, M, 1, act=act)

    def forward(self, prev_slice_weight, token):
        _refuse_bf16_storage(self.engine)
        M, C = self.M, self.C
        if prev_slice_weight.dim() != 4 or prev_slice_weight.shape[1] != 1 or prev_slice_weight.shape[-1] != M:
            raise ValueError(f"need the previous slice weights [B, 1, N, M = {M}]; got {tuple(prev_slice_weight.shape)}")
        B, _, N, _ = prev_slice_weight.shape
        if token.numel() != B * M * C:
            raise ValueError(f"need a token [B, 1, M, C] = {(B, 1, M, C)}; got {tuple(token.shape)}")
        mlp = self.weight_projection_form_slice
        first, hidden, last = mlp.linear_pre[0], mlp.linears[0][0], mlp.linear_post
        act, eng = mlp.act_name, self.engine
        # the two column blocks of the first layer's weight are cut out once per forward
        wsw, wtok = first.weight[:, :M].contiguous(), first.weight[:, M:]
        tok = token.reshape(B, M * C)
        pad = (-M * C) % 4                       # the row GEMM loads 16 bytes at a time along the contraction
        if pad:
            tok, wtok = nn.functional.pad(tok, (0, pad)), nn.functional.pad(wtok, (0, pad))
        tb = Fn.linear(tok, wtok.contiguous(), first.bias, None, engine=eng)                  # [B, H]
        h0 = Fn.prev_slice_entry(prev_slice_weight.reshape(B, N, M), wsw, tb, act, fused=self.fused_entry, engine=eng)
        y = Fn.linear(h0, hidden.weight, hidden.bias, act, engine=eng)
        h1 = y + h0 if mlp.res else y
        out = Fn.linear(h1, last.weight, last.bias, None, engine=eng)
        return out.reshape(B, 1, N, M)

    forward_previous_slice = forward
